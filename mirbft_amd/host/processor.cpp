// processor.cpp — see processor.hpp.
#include "processor.hpp"

#include <algorithm>
#include <cstring>

#include "../../include/mirsha.h"

namespace mirbft {

namespace {
[[noreturn]] void panic(mirsha_ctx* c, int rc, const char* what) {
    // The reference panics on processor failures (processor.go:75, :85, :91).
    throw std::runtime_error(std::string(what) + ": mirsha error " + std::to_string(rc) + ": " +
                             (c ? mirsha_last_error(c) : ""));
}
}  // namespace

GpuEngine::GpuEngine(int device) {
    int rc = mirsha_ctx_create(device, &ctx_);
    if (rc != MIRSHA_OK) panic(nullptr, rc, "could not create gfx950 hash engine");
}

GpuEngine::~GpuEngine() { mirsha_ctx_destroy(ctx_); }

namespace {
struct SliceLists {
    std::vector<const uint8_t*> ptr;
    std::vector<uint64_t> len;
    std::vector<uint32_t> first;
    explicit SliceLists(const std::vector<const HashRequest*>& reqs) : first(reqs.size() + 1, 0) {
        for (size_t i = 0; i < reqs.size(); i++) {
            for (const Bytes& b : reqs[i]->Data) {  // for _, data := range req.Data (processor.go:135)
                ptr.push_back(b.data);
                len.push_back(b.size);
            }
            first[i + 1] = (uint32_t)ptr.size();
        }
    }
};
}  // namespace

void GpuEngine::HashBatch(const std::vector<const HashRequest*>& reqs, std::vector<std::array<uint8_t, 32>>& out,
                          bool dedup, uint32_t* unique) {
    const uint32_t n = (uint32_t)reqs.size();
    out.resize(n);
    if (unique) *unique = n;
    if (n == 0) return;
    SliceLists sl(reqs);
    int rc = dedup ? mirsha_hash_slices_dedup(ctx_, sl.ptr.data(), sl.len.data(), sl.first.data(), n, out[0].data(),
                                              unique)
                   : mirsha_hash_slices(ctx_, sl.ptr.data(), sl.len.data(), sl.first.data(), n, out[0].data());
    if (rc != MIRSHA_OK) panic(ctx_, rc, "could not hash requests");
}

uint64_t GpuEngine::Submit(const std::vector<const HashRequest*>& reqs, std::vector<std::array<uint8_t, 32>>& out,
                           bool dedup) {
    const uint32_t n = (uint32_t)reqs.size();
    out.resize(std::max<uint32_t>(n, 1));
    SliceLists sl(reqs);
    uint64_t ticket = 0;
    int rc = mirsha_submit_slices(ctx_, sl.ptr.data(), sl.len.data(), sl.first.data(), n, out[0].data(),
                                  dedup ? MIRSHA_SUBMIT_DEDUP : 0, &ticket);
    if (rc != MIRSHA_OK) panic(ctx_, rc, "could not submit requests");
    out.resize(n);  // no reallocation: n <= capacity
    return ticket;
}

void GpuEngine::SetHasher(int hasher) {
    int rc = mirsha_ctx_set_hasher(ctx_, hasher);
    if (rc != MIRSHA_OK) panic(ctx_, rc, "could not set the hasher");
}

int GpuEngine::Hasher() const { return mirsha_ctx_hasher(ctx_); }

void GpuEngine::Wait(uint64_t ticket) {
    int rc = mirsha_wait(ctx_, ticket);
    if (rc != MIRSHA_OK) panic(ctx_, rc, "could not collect digests");
}

namespace {
class GpuSha256 final : public Hash {
public:
    explicit GpuSha256(GpuEngine& e) : e_(e) {}
    void Write(const uint8_t* p, size_t n) override { buf_.insert(buf_.end(), p, p + n); }
    std::array<uint8_t, 32> Sum() const override {
        HashRequest r;
        r.Data.push_back(Bytes{buf_.data(), buf_.size()});
        std::vector<std::array<uint8_t, 32>> out;
        e_.HashBatch({&r}, out);
        return out[0];
    }
    void Reset() override { buf_.clear(); }

private:
    GpuEngine& e_;
    std::vector<uint8_t> buf_;
};
}  // namespace

std::unique_ptr<Hash> NewGpuSha256(GpuEngine& engine) { return std::make_unique<GpuSha256>(engine); }

namespace {
ActionResults make_results(const std::vector<const HashRequest*>& reqs,
                           const std::vector<std::array<uint8_t, 32>>& digests) {
    ActionResults results;
    results.Digests.resize(reqs.size());
    for (size_t i = 0; i < reqs.size(); i++) {  // Digests[i] for actions.Hash[i] (processor.go:139)
        results.Digests[i].Request = reqs[i];
        results.Digests[i].Digest = digests[i];
    }
    return results;
}
}  // namespace

namespace {
std::vector<CheckpointResult> checkpoint_results(const std::vector<const Commit*>& commits,
                                                 const std::vector<std::array<uint8_t, 32>>& values) {
    std::vector<CheckpointResult> out;
    for (const Commit* c : commits)
        if (c->Checkpoint) {  // processor.go:164-167, commit order
            CheckpointResult r;
            r.Checkpoint = c->Checkpoint;
            r.Commit = c;
            r.Value = values.at(out.size());
            out.push_back(r);
        }
    return out;
}
}  // namespace

DeviceLog::DeviceLog(GpuEngine& engine, uint32_t n_nodes, uint32_t node)
    : engine_(engine), n_nodes_(n_nodes), node_(node) {
    if (node >= n_nodes) throw std::runtime_error("DeviceLog: node out of range");
    // the log is made with the node's Hasher (recorder.go:186-256)
    int rc = mirsha_chains_create_hasher(engine.ctx(), n_nodes, engine.Hasher(), &chains_);
    if (rc != MIRSHA_OK) panic(engine.ctx(), rc, "could not create the checkpoint chains");
}

DeviceLog::~DeviceLog() { mirsha_chains_destroy(chains_); }

namespace {
// The cycle as one programme: each non-null request digest once in the
// table, each step as n_nodes consecutive ops (node 0 first).
struct Programme {
    std::vector<uint8_t> table;
    std::vector<uint32_t> op_chain, op_digest;
    uint32_t checkpoints = 0;
};

Programme make_programme(const std::vector<const Commit*>& commits, uint32_t n_nodes) {
    Programme p;
    std::vector<uint8_t>& table = p.table;
    std::vector<uint32_t> prog;
    for (const Commit* c : commits) {
        if (!c || (c->Batch == nullptr) == (c->Checkpoint == nullptr))
            throw std::runtime_error("a Commit is a batch or else a checkpoint");
        if (c->Checkpoint) {  // value := p.Log.Snap(...) (processor.go:163)
            prog.push_back(MIRSHA_COMMIT_CHECKPOINT);
            continue;
        }
        for (const Bytes& d : c->Batch->Digests) {  // p.Log.Apply(commit.Batch) (processor.go:147)
            if (d.size == 0) {
                prog.push_back(MIRSHA_NULL_INDEX);
                continue;
            }
            if (d.size != 32 || !d.data) throw std::runtime_error("a request digest is 32 bytes, or empty");
            prog.push_back((uint32_t)(table.size() / 32));
            table.insert(table.end(), d.data, d.data + 32);
        }
    }
    for (uint32_t d : prog) {
        p.checkpoints += d == MIRSHA_COMMIT_CHECKPOINT;
        for (uint32_t node = 0; node < n_nodes; node++) {
            p.op_chain.push_back(node);
            p.op_digest.push_back(d);
        }
    }
    return p;
}
}  // namespace

std::vector<std::array<uint8_t, 32>> DeviceLog::CommitCycle(const std::vector<const Commit*>& commits) {
    const Programme p = make_programme(commits, n_nodes_);
    values_.assign((size_t)p.checkpoints * n_nodes_, {});
    uint32_t k = 0;
    int rc = mirsha_chains_commit(engine_.ctx(), chains_, p.table.data(), (uint32_t)(p.table.size() / 32),
                                  p.op_chain.data(), p.op_digest.data(), (uint32_t)p.op_chain.size(),
                                  values_.empty() ? nullptr : values_[0].data(), &k);
    if (rc != MIRSHA_OK) panic(engine_.ctx(), rc, "could not commit");
    if (k != values_.size()) throw std::runtime_error("checkpoint count mismatch");
    return Mine(values_);
}

std::vector<std::array<uint8_t, 32>> DeviceLog::Mine(const std::vector<std::array<uint8_t, 32>>& values) const {
    std::vector<std::array<uint8_t, 32>> mine(values.size() / n_nodes_);
    for (size_t j = 0; j < mine.size(); j++) mine[j] = values[j * n_nodes_ + node_];
    return mine;
}

uint64_t DeviceLog::SubmitCycle(const std::vector<const Commit*>& commits,
                                std::vector<std::array<uint8_t, 32>>& values) {
    // The library copies the programme and the table before it returns; only
    // `values` must live until the ticket retires.
    const Programme p = make_programme(commits, n_nodes_);
    values.assign((size_t)p.checkpoints * n_nodes_, {});
    uint32_t k = 0;
    uint64_t ticket = 0;
    int rc = mirsha_chains_commit_submit(engine_.ctx(), chains_, p.table.data(), (uint32_t)(p.table.size() / 32),
                                         p.op_chain.data(), p.op_digest.data(), (uint32_t)p.op_chain.size(),
                                         values.empty() ? nullptr : values[0].data(), &k, &ticket);
    if (rc != MIRSHA_OK) panic(engine_.ctx(), rc, "could not submit the commits");
    if (k != values.size()) throw std::runtime_error("checkpoint count mismatch");
    return ticket;
}

std::vector<std::array<uint8_t, 32>> DeviceLog::CollectCycle(uint64_t ticket,
                                                             const std::vector<std::array<uint8_t, 32>>& values) {
    engine_.Wait(ticket);
    values_ = values;
    return Mine(values_);
}

std::vector<CheckpointResult> Processor::CommitLoop(const Actions& actions) {
    std::vector<CheckpointResult> out;
    if (actions.Commits.empty()) return out;
    if (!log_) throw std::runtime_error("actions.Commits without an application log");  // nil p.Log
    return checkpoint_results(actions.Commits, log_->CommitCycle(actions.Commits));
}

ActionResults Processor::Process(const Actions& actions) {
    std::vector<std::array<uint8_t, 32>> digests;
    engine_.HashBatch(actions.Hash, digests, dedup_);  // one device call per Ready() cycle
    ActionResults results = make_results(actions.Hash, digests);
    results.Checkpoints = CommitLoop(actions);
    return results;
}

PendingResults Processor::Submit(const Actions& actions) {
    PendingResults p;
    p.engine_ = &engine_;
    // Applied here, ahead of the hashing (neither reads the other's results):
    // cycles commit in submission order whatever the order of the Wait calls.
    // With async_commits they are queued instead (commitInParallel beside
    // hashInParallel, processor.go:447-470) and collected by Wait.
    if (async_commits_ && !actions.Commits.empty()) {
        if (!log_) throw std::runtime_error("actions.Commits without an application log");
        p.values_ = std::make_unique<std::vector<std::array<uint8_t, 32>>>();
        p.commit_ticket_ = log_->SubmitCycle(actions.Commits, *p.values_);
        p.log_ = log_;
        p.commits_ = actions.Commits;
    } else {
        p.checkpoints_ = CommitLoop(actions);
    }
    p.reqs_ = actions.Hash;
    p.digests_ = std::make_unique<std::vector<std::array<uint8_t, 32>>>();
    if (!p.reqs_.empty()) p.ticket_ = engine_.Submit(p.reqs_, *p.digests_, dedup_);
    return p;
}

PendingResults& PendingResults::operator=(PendingResults&& o) noexcept {
    if (this != &o) {
        // overwriting an uncollected cycle: let it land first (tickets retire in order)
        if (const uint64_t last = std::max(ticket_, commit_ticket_)) {
            try { engine_->Wait(last); } catch (...) {}
        }
        engine_ = o.engine_;
        ticket_ = o.ticket_;
        commit_ticket_ = o.commit_ticket_;
        log_ = o.log_;
        commits_ = std::move(o.commits_);
        values_ = std::move(o.values_);
        o.commit_ticket_ = 0;
        reqs_ = std::move(o.reqs_);
        digests_ = std::move(o.digests_);
        checkpoints_ = std::move(o.checkpoints_);
        o.ticket_ = 0;
    }
    return *this;
}

PendingResults::~PendingResults() {
    if (const uint64_t last = std::max(ticket_, commit_ticket_)) {
        try { engine_->Wait(last); } catch (...) {}  // the buffers must outlive the library's writes
    }
}

ActionResults PendingResults::Wait() {
    if (commit_ticket_) {  // queued first, retired first
        checkpoints_ = checkpoint_results(commits_, log_->CollectCycle(commit_ticket_, *values_));
        commit_ticket_ = 0;
    }
    if (ticket_) {
        engine_->Wait(ticket_);
        ticket_ = 0;
    }
    ActionResults results = make_results(reqs_, *digests_);
    results.Checkpoints = checkpoints_;
    return results;
}

}  // namespace mirbft

extern "C" int mirbft_host_features(void) { return 1 | 2; }

extern "C" int mirbft_host_process(int device, const uint8_t* const* data, const uint64_t* len, uint32_t n,
                                   uint8_t* digests_out, char* err, uint32_t err_len) {
    return mirbft_host_process_ex(device, data, len, n, digests_out, 0, nullptr, err, err_len);
}

extern "C" int mirbft_host_process_ex(int device, const uint8_t* const* data, const uint64_t* len, uint32_t n,
                                      uint8_t* digests_out, int flags, uint32_t* unique_out, char* err,
                                      uint32_t err_len) {
    try {
        mirbft::GpuEngine engine(device);
        if (flags & 8) engine.SetHasher(MIRSHA_HASHER_SHA512_256);
        mirbft::Processor p(engine, (flags & 1) != 0);
        std::vector<mirbft::HashRequest> reqs(n);
        mirbft::Actions a;
        for (uint32_t i = 0; i < n; i++) {
            reqs[i].Data.push_back(mirbft::Bytes{data[i], (size_t)len[i]});
            a.Hash.push_back(&reqs[i]);
        }
        mirbft::ActionResults r;
        if (flags & 4) {
            // A cycle dropped without Wait, then 4 more: the ring retires the
            // dropped one while later submissions are queued.
            { mirbft::PendingResults dropped = p.Submit(a); }
            std::vector<mirbft::PendingResults> more;
            for (int k = 0; k < 4; k++) more.push_back(p.Submit(a));
            for (auto& m : more) r = m.Wait();
        } else if (flags & 2) {
            mirbft::PendingResults pending = p.Submit(a);
            r = pending.Wait();
        } else {
            r = p.Process(a);
        }
        if (unique_out) {
            std::vector<std::array<uint8_t, 32>> tmp;
            *unique_out = n;
            if (flags & 1) engine.HashBatch(a.Hash, tmp, true, unique_out);
        }
        for (uint32_t i = 0; i < n; i++) {
            if (r.Digests[i].Request != &reqs[i]) throw std::runtime_error("origin order violated");
            memcpy(digests_out + 32ull * i, r.Digests[i].Digest.data(), 32);
        }
        return 0;
    } catch (const std::exception& e) {
        if (err && err_len) {
            strncpy(err, e.what(), err_len - 1);
            err[err_len - 1] = 0;
        }
        return -1;
    }
}

extern "C" int mirbft_host_commit(int device, uint32_t n_nodes, const uint8_t* const* digest_ptr,
                                  const uint32_t* batch_len, uint32_t n_commits, uint8_t* values_out,
                                  uint32_t* n_checkpoints_out, int flags, char* err, uint32_t err_len) {
    try {
        mirbft::GpuEngine engine(device);
        if (flags & 8) engine.SetHasher(MIRSHA_HASHER_SHA512_256);  // before the log is made: it takes the engine's
        mirbft::DeviceLog log(engine, n_nodes);
        mirbft::Processor p(engine, false, &log, (flags & 4) != 0);
        std::vector<mirbft::CommitBatch> batches(n_commits);
        std::vector<mirbft::Checkpoint> cps(n_commits);
        std::vector<mirbft::Commit> commits(n_commits);
        mirbft::Actions a;
        size_t at = 0;
        for (uint32_t i = 0; i < n_commits; i++) {
            if (batch_len[i] == UINT32_MAX) {
                cps[i].SeqNo = i;
                commits[i].Checkpoint = &cps[i];
            } else {
                for (uint32_t k = 0; k < batch_len[i]; k++, at++)
                    batches[i].Digests.push_back(mirbft::Bytes{digest_ptr[at], digest_ptr[at] ? (size_t)32 : 0});
                commits[i].Batch = &batches[i];
            }
            a.Commits.push_back(&commits[i]);
        }
        mirbft::ActionResults r;
        if (flags & 2) {
            mirbft::PendingResults pending = p.Submit(a);
            if (pending.CommitsQueued() != ((flags & 4) != 0 && n_commits != 0))
                throw std::runtime_error("the commits were not queued as the option says");
            r = pending.Wait();
        } else {
            r = p.Process(a);
        }
        size_t j = 0;
        for (uint32_t i = 0; i < n_commits; i++)
            if (commits[i].Checkpoint) {
                if (j >= r.Checkpoints.size() || r.Checkpoints[j].Commit != &commits[i] ||
                    r.Checkpoints[j].Checkpoint != &cps[i])
                    throw std::runtime_error("commit order violated");
                if (memcmp(r.Checkpoints[j].Value.data(), log.Values()[j * n_nodes].data(), 32) != 0)
                    throw std::runtime_error("node 0's value differs from the log's");
                j++;
            }
        if (j != r.Checkpoints.size()) throw std::runtime_error("checkpoint count mismatch");
        for (size_t v = 0; v < log.Values().size(); v++) memcpy(values_out + 32 * v, log.Values()[v].data(), 32);
        if (n_checkpoints_out) *n_checkpoints_out = (uint32_t)j;
        return 0;
    } catch (const std::exception& e) {
        if (err && err_len) {
            strncpy(err, e.what(), err_len - 1);
            err[err_len - 1] = 0;
        }
        return -1;
    }
}
