// processor.hpp — C++ host mirror of the reference's Processor hash path
// (Go package github.com/IBM/mirbft; no Go toolchain in this image, so the
// host side above the C-ABI is C++, with the reference's names and semantics).
//
//   reference                                   here
//   type Hasher func() hash.Hash  processor.go:21     mirbft::Hasher (factory of mirbft::Hash)
//   HashRequest{Data [][]byte; Origin}  actions.go:157-164   mirbft::HashRequest
//   HashResult{Digest; Request}         actions.go:224-230   mirbft::HashResult
//   ActionResults{Digests; ...}         actions.go:218-221   mirbft::ActionResults
//   (*Processor).Process hash loop      processor.go:129-143 mirbft::Processor::Process
//   Commit{Batch; Checkpoint}           actions.go:169-179   mirbft::Commit
//   CheckpointResult{Checkpoint; Value} actions.go:234-243   mirbft::CheckpointResult
//   (*Processor).Process commit loop    processor.go:145-168 mirbft::Processor (with a mirbft::DeviceLog)
//
// Processor::Process coalesces every HashRequest of one Ready() cycle into ONE
// batched device call (mirsha_hash_slices) and returns Digests[i] for
// actions.Hash[i] with the Request back-pointer, in origin order.  Failures
// throw std::runtime_error — the reference panics (processor.go:75,81,85,91).
// Options: dedup (hash each distinct request content once per cycle,
// mirsha_hash_slices_dedup) and the asynchronous Submit / Pending::Wait form
// (mirsha_submit_slices / mirsha_wait) for overlapping the cycle's hashing
// with its WAL writes and sends, as ProcessorWorkPool does (processor.go:447-470).
// The commit loop: a cycle's actions.Commits go to the Processor's DeviceLog in
// ONE mirsha_chains_commit call and ActionResults.Checkpoints holds one
// CheckpointResult per checkpoint, in commit order; Commits without a log throw.
#pragma once
#include <array>
#include <cstdint>
#include <functional>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

struct mirsha_ctx;
struct mirsha_chains;

namespace mirbft {

struct Bytes {
    const uint8_t* data = nullptr;
    size_t size = 0;
};

// Origin is opaque to the hasher (actions.go:152-156): carried, never read.
struct HashRequest {
    std::vector<Bytes> Data;
    const void* Origin = nullptr;
};

struct HashResult {
    std::array<uint8_t, 32> Digest{};
    const HashRequest* Request = nullptr;
};

// mirbft.Checkpoint (actions.go:192-205); opaque to the log.
struct Checkpoint {
    uint64_t SeqNo = 0;
    const void* NetworkConfig = nullptr;
    const void* ClientsState = nullptr;
};

// What the application log reads of a committed pb.QEntry: each request's
// digest in order (recorder.go:222-223); size 0 = a null request.
struct CommitBatch {
    uint64_t SeqNo = 0;
    std::vector<Bytes> Digests;
};

// mirbft.Commit (actions.go:169-179): a batch, or else a checkpoint.
struct Commit {
    const CommitBatch* Batch = nullptr;
    const struct Checkpoint* Checkpoint = nullptr;
};

struct CheckpointResult {
    const struct Checkpoint* Checkpoint = nullptr;  // the request that asked for it (actions.go:236)
    const struct Commit* Commit = nullptr;
    std::array<uint8_t, 32> Value{};
};

struct Actions {
    std::vector<const HashRequest*> Hash;  // actions.go:24
    std::vector<const Commit*> Commits;    // actions.go:38
};

struct ActionResults {
    std::vector<HashResult> Digests;            // actions.go:219
    std::vector<CheckpointResult> Checkpoints;  // actions.go:220
};

// Streaming hash.Hash (Write/Sum/Reset) for single-message callers.
class Hash {
public:
    virtual ~Hash() = default;
    virtual void Write(const uint8_t* p, size_t n) = 0;
    virtual std::array<uint8_t, 32> Sum() const = 0;
    virtual void Reset() = 0;
};
using Hasher = std::function<std::unique_ptr<Hash>()>;

// One gfx950 engine (device context); the batched replacement for Hasher.
class GpuEngine {
public:
    explicit GpuEngine(int device = 0);
    ~GpuEngine();
    GpuEngine(const GpuEngine&) = delete;
    GpuEngine& operator=(const GpuEngine&) = delete;

    // Digests of reqs[i] (concat of its Data slices) at out[i], origin order.
    // dedup: identical requests are hashed once; *unique = distinct requests.
    void HashBatch(const std::vector<const HashRequest*>& reqs, std::vector<std::array<uint8_t, 32>>& out,
                   bool dedup = false, uint32_t* unique = nullptr);
    // Asynchronous form: packs reqs before returning; `out` (resized here) is
    // filled, in origin order, by Wait(ticket).
    uint64_t Submit(const std::vector<const HashRequest*>& reqs, std::vector<std::array<uint8_t, 32>>& out,
                    bool dedup = false);
    void Wait(uint64_t ticket);
    // The reference's `Hasher` (processor.go:21,58) of the calls made from now
    // on: MIRSHA_HASHER_SHA256 (default) or MIRSHA_HASHER_SHA512_256
    // (mirsha_ctx_set_hasher).  A DeviceLog takes the engine's hasher when it is
    // made: set the hasher first.  A log made under another hasher than the
    // engine has at a commit panics there.
    void SetHasher(int hasher);
    int Hasher() const;
    mirsha_ctx* ctx() { return ctx_; }

private:
    mirsha_ctx* ctx_ = nullptr;
};

// hash.Hash whose Sum runs on the GPU (buffers its writes).
std::unique_ptr<Hash> NewGpuSha256(GpuEngine& engine);

// The application log on the device: it stands where p.Log.Apply / p.Log.Snap
// stand (processor.go:147,163), the testengine application's state
// (NodeState.ActiveHash, recorder.go:186-256) in a mirsha_chains.  n_nodes = 1:
// a node's own log (chain 0); n_nodes > 1: a testengine-style log, all nodes
// commit the cycle's entries (the digest table is passed once).  The chains
// hash with the engine's Hasher() as it is at construction
// (mirsha_chains_create_hasher).
class DeviceLog {
public:
    explicit DeviceLog(GpuEngine& engine, uint32_t n_nodes = 1, uint32_t node = 0);
    ~DeviceLog();
    DeviceLog(const DeviceLog&) = delete;
    DeviceLog& operator=(const DeviceLog&) = delete;
    // One cycle's commits in ONE mirsha_chains_commit call; node `node`'s value
    // per checkpoint, in commit order.  Values(): every node's, row
    // checkpoint * n_nodes + node.
    std::vector<std::array<uint8_t, 32>> CommitCycle(const std::vector<const Commit*>& commits);
    const std::vector<std::array<uint8_t, 32>>& Values() const { return values_; }
    // The asynchronous form (mirsha_chains_commit_submit): the cycle is queued
    // as a ticket of the engine's ring and the call returns.  `values` (sized
    // here, every node's rows) is written until the ticket retires and must
    // live that long; CollectCycle waits for the ticket and returns what
    // CommitCycle would have (Values() then holds that cycle's).  Cycles take
    // effect in submission order, whatever the order they are collected in.
    uint64_t SubmitCycle(const std::vector<const Commit*>& commits, std::vector<std::array<uint8_t, 32>>& values);
    std::vector<std::array<uint8_t, 32>> CollectCycle(uint64_t ticket,
                                                      const std::vector<std::array<uint8_t, 32>>& values);

private:
    std::vector<std::array<uint8_t, 32>> Mine(const std::vector<std::array<uint8_t, 32>>& values) const;
    GpuEngine& engine_;
    mirsha_chains* chains_ = nullptr;
    uint32_t n_nodes_, node_;
    std::vector<std::array<uint8_t, 32>> values_;
};

// One submitted cycle; Wait() returns its ActionResults (origin order).
// Owns the buffer the library writes the digests into (inside mirsha_wait, or
// when a later submission retires this one's ring slot), so it is move-only
// and its destructor waits for a cycle that was never collected.
class PendingResults {
public:
    PendingResults() = default;
    PendingResults(PendingResults&& o) noexcept { *this = std::move(o); }
    PendingResults& operator=(PendingResults&& o) noexcept;
    PendingResults(const PendingResults&) = delete;
    PendingResults& operator=(const PendingResults&) = delete;
    ~PendingResults();
    ActionResults Wait();
    // async_commits: the cycle's commits are a ring ticket not yet collected.
    bool CommitsQueued() const { return commit_ticket_ != 0; }

private:
    friend class Processor;
    GpuEngine* engine_ = nullptr;
    uint64_t ticket_ = 0;
    std::vector<const HashRequest*> reqs_;
    std::unique_ptr<std::vector<std::array<uint8_t, 32>>> digests_;
    std::vector<CheckpointResult> checkpoints_;  // the commits were applied at Submit
    // async_commits: the cycle's commit ticket, its Commits, and the buffer the
    // library writes the checkpoint values into until that ticket retires.
    uint64_t commit_ticket_ = 0;
    DeviceLog* log_ = nullptr;
    std::vector<const Commit*> commits_;
    std::unique_ptr<std::vector<std::array<uint8_t, 32>>> values_;
};

class Processor {
public:
    // async_commits: Submit queues the cycle's commits (DeviceLog::SubmitCycle)
    // ahead of its hashing instead of applying them first; Wait collects
    // them.  The ActionResults are the same either way.
    explicit Processor(GpuEngine& engine, bool dedup = false, DeviceLog* log = nullptr, bool async_commits = false)
        : engine_(engine), dedup_(dedup), log_(log), async_commits_(async_commits) {}
    // processor.go:129-143, batched; then the commit loop (:145-168) in one call.
    ActionResults Process(const Actions& actions);
    // Asynchronous Process: queue the cycle's hashing and return at once.
    PendingResults Submit(const Actions& actions);

private:
    std::vector<CheckpointResult> CommitLoop(const Actions& actions);
    GpuEngine& engine_;
    bool dedup_;
    DeviceLog* log_;
    bool async_commits_;
};

}  // namespace mirbft

extern "C" {
// What this build of the mirror offers beyond the first C entries: bit 0 = the
// Processor's async_commits option (bit 2 of mirbft_host_commit's flags), bit 1
// = the log's hasher (bit 3 of mirbft_host_commit's flags).
int mirbft_host_features(void);
// Small C entry for tests: hash n single-slice requests through
// mirbft::Processor (exercises the C++ mirror end to end).
int mirbft_host_process(int device, const uint8_t* const* data, const uint64_t* len, uint32_t n,
                        uint8_t* digests_out, char* err, uint32_t err_len);
// flags: bit 0 = dedup, bit 1 = asynchronous (Submit, then Wait), bit 2 =
// asynchronous with a dropped (never waited) cycle before four more, bit 3 =
// the engine's hasher is MIRSHA_HASHER_SHA512_256 (GpuEngine::SetHasher).
int mirbft_host_process_ex(int device, const uint8_t* const* data, const uint64_t* len, uint32_t n,
                           uint8_t* digests_out, int flags, uint32_t* unique_out, char* err, uint32_t err_len);
// One cycle's commits through mirbft::Processor with an n_nodes DeviceLog:
// commit i is a batch of batch_len[i] requests whose digests are the next
// batch_len[i] entries of digest_ptr (32 bytes each; NULL = a null request), or
// a checkpoint if batch_len[i] == UINT32_MAX.  values_out: 32 bytes per
// checkpoint and node (row checkpoint * n_nodes + node); flags bit 1 =
// asynchronous (Submit, then Wait), bit 2 = the Processor's async_commits
// option (with bit 1: the commits are a ring ticket of their own), bit 3 =
// the engine's hasher, and so the log's, is MIRSHA_HASHER_SHA512_256.
int mirbft_host_commit(int device, uint32_t n_nodes, const uint8_t* const* digest_ptr, const uint32_t* batch_len,
                       uint32_t n_commits, uint8_t* values_out, uint32_t* n_checkpoints_out, int flags, char* err,
                       uint32_t err_len);
}
