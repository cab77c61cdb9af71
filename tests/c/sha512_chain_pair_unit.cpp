// CPU unit test of mirbft_amd/csrc/sha512_chain_pair.h (no HIP): a commit
// programme's step split into a producer (the walk, the block, the schedule) and
// a consumer (the rounds, the state, a checkpoint's row), for 64 lanes in
// lock-step through a host array shaped like the ring of
// mirsha_sha512_chains_pair.hip.
//
// The two roles are written as the kernels' two waves see the loop, each a
// routine of its own that runs up to its next barrier; the driver lets both run
// one phase (the stretch between two barriers) at a time and requires that both
// reach a barrier or both have left the loop: the same number of barriers on
// every input.  Every ring slot and control word carries the phase of its last
// writing and reading: a read must find something written in an EARLIER phase
// (the two waves run a phase concurrently on the device) and not yet consumed,
// a write must find what it overwrites consumed in an earlier phase.
//
// Expected values: the walk of the one-lane kernels (chain_walk,
// mirsha_sha512_chains.hip) with sha512::chain_plan / chain_block / compress,
// per lane: every checkpoint row, and the final h, cnt and pending words below
// cnt % 4.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "sha512_chain_pair.h"

namespace s5 = mirsha::sha512;

static constexpr uint32_t kLanes = 64;
static constexpr uint32_t CP = s5::kChainCheckpoint;

#define REQUIRE(cond, ...)                \
    do {                                  \
        if (!(cond)) {                    \
            fprintf(stderr, __VA_ARGS__); \
            fprintf(stderr, "\n");        \
            exit(1);                      \
        }                                 \
    } while (0)

static uint64_t rnd(uint64_t& s) {  // splitmix64
    uint64_t z = (s += 0x9e3779b97f4a7c15ull);
    z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
    z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
    return z ^ (z >> 31);
}

// The digest table: row r, as its 8 dwords lie in memory.
static void table_row(uint32_t r, uint32_t row[8]) {
    uint8_t b[32];
    for (uint32_t j = 0; j < 32; j++) b[j] = (uint8_t)(r * 37u + j * 11u + (r >> 8) * 3u + 5u);
    memcpy(row, b, 32);
}

// A chain's state and its programme.
struct Lane {
    uint64_t h[8], pend[s5::kChainPendWords], cnt;
    std::vector<uint32_t> ent;
};

struct Fetch {
    s5::ChainStep s;
    uint32_t rows[4][8];
};

// The loads of a step, as the kernels guard them: an entry only inside the
// lane's range, a row only where the plan takes it.  Everything else holds
// garbage that must not show.
static void load_entries(const Lane& l, uint32_t e, uint32_t x[4]) {
    for (uint32_t i = 0; i < 4; i++) x[i] = e + i < l.ent.size() ? l.ent[e + i] : 0xFFFFFFFFu;
}
static void load_rows(Fetch& f) {
    for (int sl = 0; sl < 4; sl++) {
        for (auto& d : f.rows[sl]) d = 0xDEADBEEFu;
        if ((f.s.take >> sl) & 1u) table_row(f.s.id[sl], f.rows[sl]);
    }
}

// ---- the reference: one lane, one wave ------------------------------------------

struct Want {
    uint64_t h[8], pend[s5::kChainPendWords], cnt;
    uint32_t compressions = 0;
};

static Want reference(const Lane& l, std::vector<uint8_t>& out) {
    Want r;
    memcpy(r.h, l.h, sizeof r.h);
    memcpy(r.pend, l.pend, sizeof r.pend);
    uint64_t n = l.cnt;
    uint32_t e = 0;
    const uint32_t end = (uint32_t)l.ent.size();
    for (;;) {
        uint32_t x[4];
        load_entries(l, e, x);
        Fetch f;
        f.s = s5::chain_plan(x, end - e, n);
        if (!(f.s.full || f.s.cp || f.s.keep)) break;
        load_rows(f);
        e += f.s.consumed;
        n = f.s.n_after;
        uint64_t w[16];
        s5::chain_block(r.pend, f.rows, f.s, w);
        if (f.s.keep) s5::chain_keep(w, r.pend);
        if (f.s.full || f.s.cp) {
            s5::compress(r.h, w);
            r.compressions++;
        }
        if (f.s.cp) {
            uint32_t d[8];
            s5::digest_words(r.h, d);
            REQUIRE(32ull * f.s.row + 32u <= out.size(), "reference: row %u out of range", f.s.row);
            memcpy(out.data() + 32ull * f.s.row, d, 32);
            memcpy(r.h, s5::kH0, sizeof r.h);
        }
    }
    REQUIRE(e == end, "reference: %u of %u entries walked", e, end);
    r.cnt = n;
    return r;
}

// ---- the ring with its stamps ----------------------------------------------------

struct Ring {
    uint64_t kw[2][kLanes][16];
    long kw_written[2] = {-1, -1}, kw_read[2] = {-1, -1};
    bool kw_unread[2] = {false, false};
    uint32_t ctl[2][kLanes], more[2];
    long cw_written[2] = {-1, -1}, cw_read[2] = {-1, -1};
    int more_readers[2] = {2, 2};  // both roles read a step's "another step"
    long phase = 0;                // barriers passed by both roles

    void write_slot(uint32_t s) {
        REQUIRE(!kw_unread[s], "phase %ld: slot %u rewritten before it was read", phase, s);
        REQUIRE(kw_read[s] < phase, "phase %ld: slot %u written in the phase of its reading", phase, s);
        kw_written[s] = phase;
        kw_unread[s] = true;
    }
    void read_slot(uint32_t s) {
        REQUIRE(kw_unread[s], "phase %ld: slot %u read twice or never written", phase, s);
        REQUIRE(kw_written[s] < phase, "phase %ld: slot %u read in the phase of its writing", phase, s);
        kw_read[s] = phase;
        kw_unread[s] = false;
    }
    void consumed(uint32_t s) {  // whoever reads it again reads garbage
        for (auto& lane : kw[s])
            for (auto& x : lane) x = 0xDEADBEEFDEADBEEFull;
    }
    void write_control(uint32_t i) {
        REQUIRE(more_readers[i] == 2, "phase %ld: control %u rewritten before both roles read it", phase, i);
        REQUIRE(cw_read[i] < phase, "phase %ld: control %u written in the phase of its reading", phase, i);
        cw_written[i] = phase;
        more_readers[i] = 0;
    }
    void read_control(uint32_t i) {
        REQUIRE(more_readers[i] < 2 && cw_written[i] >= 0, "phase %ld: control %u read but not written", phase, i);
        REQUIRE(cw_written[i] < phase, "phase %ld: control %u read in the phase of its writing", phase, i);
        cw_read[i] = phase;
        more_readers[i]++;
    }
};

// ---- the producer (wave 0) ----------------------------------------------------------

struct Producer {
    const std::vector<Lane>& lanes;
    Ring& ring;
    struct PLane {
        uint32_t e = 0, end = 0, x[4];
        uint64_t n = 0, pw[s5::kChainPendWords], w[16];
        Fetch nxt;
    } pl[kLanes];
    uint32_t t = 0;
    int g = -2;  // -2: before the loop, -1: at the loop's top, 0..4: the group to do
    long barriers = 0;

    Producer(const std::vector<Lane>& l, Ring& r) : lanes(l), ring(r) {}

    void fetch(uint32_t k, Fetch& f) {
        PLane& p = pl[k];
        f.s = s5::chain_pair_plan(p.x, p.end, p.e, p.n);
        load_rows(f);
        load_entries(lanes[k], p.e, p.x);
    }
    void open_step(uint32_t step, uint32_t slot) {
        uint32_t ctl[kLanes];
        bool any = false;
        for (uint32_t k = 0; k < kLanes; k++) {
            PLane& p = pl[k];
            const Fetch cur = p.nxt;
            fetch(k, p.nxt);
            ctl[k] = s5::chain_pair_produce(p.pw, cur.rows, cur.s, p.w);
            any = any || s5::chain_pair_live(ctl[k]);  // the ballot
        }
        ring.write_control(step & 1u);
        memcpy(ring.ctl[step & 1u], ctl, sizeof ctl);
        ring.more[step & 1u] = any ? 1u : 0u;
        if (any) put<0>(slot);
    }
    template <int G>
    void put(uint32_t slot) {
        ring.write_slot(slot);
        for (uint32_t k = 0; k < kLanes; k++) s5::produce_group<G>(pl[k].w, ring.kw[slot][k]);
    }
    // Runs to the next barrier; false: left the loop.
    bool run() {
        if (g == -2) {
            for (uint32_t k = 0; k < kLanes; k++) {
                PLane& p = pl[k];
                memcpy(p.pw, lanes[k].pend, sizeof p.pw);
                p.n = lanes[k].cnt;
                p.end = (uint32_t)lanes[k].ent.size();
                load_entries(lanes[k], 0u, p.x);
                fetch(k, p.nxt);
            }
            open_step(0u, 0u);
            g = -1;
            barriers++;
            return true;
        }
        if (g == -1) {
            ring.read_control(t & 1u);
            if (!ring.more[t & 1u]) return false;
            g = 0;
        }
        const uint32_t rd = (t + (uint32_t)g) & 1u, wr = rd ^ 1u;
        switch (g) {
        case 0: put<1>(wr); break;
        case 1: put<2>(wr); break;
        case 2: put<3>(wr); break;
        case 3: put<4>(wr); break;
        default: open_step(t + 1u, wr); break;
        }
        if (++g == s5::kPairGroups) {
            g = -1;
            t++;
        }
        barriers++;
        return true;
    }
};

// ---- the consumer (wave 1) ----------------------------------------------------------

struct Consumer {
    Ring& ring;
    std::vector<uint8_t>& out;
    struct CLane {
        uint64_t st[8], v[8];
        uint32_t ctl = 0;
    } cl[kLanes];
    uint32_t t = 0;
    int g = -2;
    bool finish = false;  // the end of step t - 1 is still to do
    long barriers = 0;
    uint32_t steps = 0;

    Consumer(const std::vector<Lane>& lanes, Ring& r, std::vector<uint8_t>& o) : ring(r), out(o) {
        for (uint32_t k = 0; k < kLanes; k++) memcpy(cl[k].st, lanes[k].h, sizeof cl[k].st);
    }
    bool run() {
        if (g == -2) {
            g = -1;
            barriers++;
            return true;
        }
        if (finish) {
            for (uint32_t k = 0; k < kLanes; k++) {
                uint32_t d[8];
                if (s5::chain_pair_finish(cl[k].st, cl[k].v, cl[k].ctl, d)) {
                    const uint32_t row = s5::chain_pair_row(cl[k].ctl);
                    REQUIRE(32ull * row + 32u <= out.size(), "lane %u: row %u out of range", k, row);
                    memcpy(out.data() + 32ull * row, d, 32);
                }
            }
            finish = false;
        }
        if (g == -1) {
            ring.read_control(t & 1u);
            if (!ring.more[t & 1u]) return false;
            for (uint32_t k = 0; k < kLanes; k++) {
                cl[k].ctl = ring.ctl[t & 1u][k];
                memcpy(cl[k].v, cl[k].st, sizeof cl[k].v);
            }
            g = 0;
        }
        const uint32_t rd = (t + (uint32_t)g) & 1u;
        ring.read_slot(rd);
        for (uint32_t k = 0; k < kLanes; k++) s5::consume_group(cl[k].v, ring.kw[rd][k]);
        ring.consumed(rd);
        if (++g == s5::kPairGroups) {
            g = -1;
            t++;
            steps++;
            finish = true;
        }
        barriers++;
        return true;
    }
};

// ---- one group of 64 programmes -----------------------------------------------------

static long groups_run = 0;

static void run_group(const char* what, std::vector<Lane> lanes, uint32_t n_rows) {
    REQUIRE(lanes.size() <= kLanes, "%s: too many lanes", what);
    lanes.resize(kLanes);  // the rest: fresh chains without entries
    std::vector<uint8_t> want_out(32ull * n_rows + 32u, 0xEE), got_out(want_out);
    std::vector<Want> want;
    uint32_t steps = 0;
    for (const Lane& l : lanes) {
        want.push_back(reference(l, want_out));
        if (want.back().compressions > steps) steps = want.back().compressions;
    }
    Ring ring;
    Producer prod(lanes, ring);
    Consumer cons(lanes, ring, got_out);
    for (;;) {
        // the two roles run a phase concurrently: neither order may matter, so alternate
        bool p, c;
        if (ring.phase & 1) {
            c = cons.run();
            p = prod.run();
        } else {
            p = prod.run();
            c = cons.run();
        }
        REQUIRE(p == c, "%s: phase %ld: the %s left the loop alone", what, ring.phase, p ? "consumer" : "producer");
        if (!p) break;
        ring.phase++;
    }
    REQUIRE(prod.barriers == cons.barriers, "%s: barriers %ld / %ld", what, prod.barriers, cons.barriers);
    REQUIRE(prod.barriers == 1 + 5l * steps && cons.steps == steps, "%s: %ld barriers, %u steps, %u expected", what,
            prod.barriers, cons.steps, steps);
    REQUIRE(got_out == want_out, "%s: checkpoint rows differ", what);
    for (uint32_t k = 0; k < kLanes; k++) {
        const Want& w = want[k];
        REQUIRE(memcmp(cons.cl[k].st, w.h, sizeof w.h) == 0, "%s: lane %u: h differs", what, k);
        REQUIRE(prod.pl[k].n == w.cnt, "%s: lane %u: cnt %llu, %llu expected", what, k,
                (unsigned long long)prod.pl[k].n, (unsigned long long)w.cnt);
        REQUIRE(memcmp(prod.pl[k].pw, w.pend, 32u * (w.cnt & 3u)) == 0, "%s: lane %u: pending words differ", what, k);
        REQUIRE(prod.pl[k].e == lanes[k].ent.size(), "%s: lane %u: entries left", what, k);
    }
    groups_run++;
}

// ---- inputs -------------------------------------------------------------------------

static Lane fresh() {
    Lane l;
    memcpy(l.h, s5::kH0, sizeof l.h);
    memset(l.pend, 0, sizeof l.pend);
    l.cnt = 0;
    return l;
}

// A chain in the middle of a message: p rows pending, any midstate, garbage
// in the pending words past the p rows.
static Lane lane_with_pending(uint64_t& seed, uint32_t p) {
    Lane l;
    for (auto& x : l.h) x = rnd(seed);
    for (auto& x : l.pend) x = rnd(seed);
    l.cnt = 4ull * (rnd(seed) % 1000u) + p;
    if (p == 0 && (rnd(seed) & 1u)) {
        memcpy(l.h, s5::kH0, sizeof l.h);
        l.cnt = 0;
    }
    return l;
}

static uint32_t a_row(uint64_t& seed) { return (uint32_t)(rnd(seed) % 5000u); }

// Every pending count against every kind of step: the classes as lanes of one
// group, and each alone beside 63 lanes without entries.
static void step_classes() {
    uint64_t seed = 0x636861696e706172ull;
    struct Class {
        uint32_t p;
        std::vector<uint32_t> kinds;  // 0: a write, 1: a checkpoint
    };
    std::vector<Class> classes;
    for (uint32_t p = 0; p < 4; p++) {
        classes.push_back({p, std::vector<uint32_t>(4u - p, 0u)});  // a full block
        for (uint32_t j = 0; j + p <= 3; j++) {
            std::vector<uint32_t> k(j, 0u);
            classes.push_back({p, k});  // the lane's end after j writes (j = 0: no entry at all)
            k.push_back(1u);
            classes.push_back({p, k});  // a checkpoint after j writes
            // ... and the same behind a full block, so the class is not the lane's first step
            std::vector<uint32_t> behind(4u - p, 0u);
            behind.insert(behind.end(), k.begin(), k.end());
            classes.push_back({p, behind});
        }
    }
    REQUIRE(classes.size() <= kLanes, "step classes: %zu lanes", classes.size());
    std::vector<Lane> together;
    uint32_t rows = 0;
    for (const Class& c : classes) {
        Lane l = lane_with_pending(seed, c.p);
        for (uint32_t kind : c.kinds) l.ent.push_back(kind ? CP | rows++ : a_row(seed));
        together.push_back(l);
    }
    run_group("step classes in one group", together, rows);
    for (Lane l : together) {
        uint32_t alone_rows = 0;
        for (auto& x : l.ent)
            if (x & CP) x = CP | alone_rows++;
        std::vector<Lane> g(17, fresh());  // lane 17: no special place in the wave
        g.push_back(l);
        run_group("a step class alone", g, alone_rows);
    }
}

static void consecutive_checkpoints() {
    uint64_t seed = 0x6370637063706370ull;
    std::vector<Lane> g;
    uint32_t rows = 0;
    for (uint32_t p = 0; p < 4; p++)
        for (uint32_t run = 2; run <= 5; run++) {
            Lane l = lane_with_pending(seed, p);
            if (run & 1u) l.ent.push_back(a_row(seed));
            for (uint32_t i = 0; i < run; i++) l.ent.push_back(CP | rows++);
            if (p & 1u) {
                l.ent.push_back(a_row(seed));
                l.ent.push_back(CP | rows++);
                l.ent.push_back(CP | rows++);
            }
            g.push_back(l);
        }
    run_group("consecutive checkpoints", g, rows);
}

static void empty_programme() {
    run_group("no entries, fresh chains", {}, 0);
    uint64_t seed = 0x656d707479ull;
    std::vector<Lane> g;
    for (uint32_t k = 0; k < kLanes; k++) g.push_back(lane_with_pending(seed, k & 3u));
    run_group("no entries, chains with state", g, 0);
}

static void random_groups() {
    uint64_t seed = 0x72616e646f6d3634ull;
    for (int trial = 0; trial < 200; trial++) {
        std::vector<Lane> g;
        uint32_t rows = 0;
        const uint32_t cp_in = 2u + (uint32_t)(rnd(seed) % 9u);  // a checkpoint one entry in 2..10
        for (uint32_t k = 0; k < kLanes; k++) {
            Lane l = lane_with_pending(seed, (uint32_t)(rnd(seed) & 3u));
            const uint32_t len = (uint32_t)(rnd(seed) % 41u);
            for (uint32_t i = 0; i < len; i++) l.ent.push_back(rnd(seed) % cp_in == 0u ? CP | rows++ : a_row(seed));
            g.push_back(l);
        }
        // rows in any order over the lanes: an output row is named by its entry alone
        std::vector<uint32_t> perm(rows);
        for (uint32_t i = 0; i < rows; i++) perm[i] = i;
        for (uint32_t i = rows; i > 1; i--) std::swap(perm[i - 1], perm[rnd(seed) % i]);
        for (Lane& l : g)
            for (auto& x : l.ent)
                if (x & CP) x = CP | perm[x & ~CP];
        run_group("random group", g, rows);
    }
}

int main() {
    // the control word keeps a checkpoint's row and never mistakes a whole block for one
    s5::ChainStep s = {};
    s.full = true;
    REQUIRE(s5::chain_pair_ctl(s) == s5::kChainPairLive && !s5::chain_pair_cp(s5::kChainPairLive), "control: full");
    s.full = false;
    s.cp = true;
    for (uint32_t row : {0u, 1u, 0x7FFFFFFFu}) {
        s.row = row;
        const uint32_t ctl = s5::chain_pair_ctl(s);
        REQUIRE(s5::chain_pair_live(ctl) && s5::chain_pair_cp(ctl) && s5::chain_pair_row(ctl) == row, "control: row %u",
                row);
    }
    s.cp = false;
    s.keep = true;
    REQUIRE(!s5::chain_pair_live(s5::chain_pair_ctl(s)), "control: keep");
    step_classes();
    consecutive_checkpoints();
    empty_programme();
    random_groups();
    printf("sha512 chain pair unit ok: %ld groups\n", groups_run);
    return 0;
}
