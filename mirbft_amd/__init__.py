"""mirbft_amd — MI355X-native engine for MirBFT's Actions.Hash hot path.

Drop-in for the hash loop of the reference Processor (processor.go:129-143):
SHA-256 request, batch, VerifyBatch, epoch-change and checkpoint digests,
bit-exact with Go crypto/sha256, returned in origin order.  All compute runs in
hand-written gfx950 HIP kernels behind the C-ABI in include/mirsha.h.
"""
from . import eventlog, hashdata, sharding
from ._lib import MirshaError, MirshaUnavailable
from .engine import (STREAM_RESET, STREAM_SUM, STREAM_SUM_RESET, STREAM_WRITE, CheckpointChains, CommitTicket, Engine,
                     ExpectTicket, HASHERS, HashStreams, MultiEngine, SliceArrays, StreamHasher, StreamTicket, Ticket, bucket_order, commit_plan,
                     commit_seg_plan, dedup_plan, dedup_rows, device_count, expect_bitmap, expect_plan, hash_batch_multi,
                     hasher_info, mismatch_indices, order_plan, stream_plan, stream_seg_plan)
from .processor import (ActionResults, Actions, Checkpoint, CheckpointResult, Commit, CommitBatch, DeviceLog, GpuHash,
                        HashRequest, HashResult, PendingResults, Processor, ProcessorWorkPool, StreamLog,
                        commit_programme, gpu_hasher)

__all__ = [
    "Engine",
    "CheckpointChains",
    "HashStreams",
    "StreamHasher",
    "StreamLog",
    "stream_plan",
    "stream_seg_plan",
    "STREAM_WRITE",
    "STREAM_SUM",
    "STREAM_SUM_RESET",
    "STREAM_RESET",
    "SliceArrays",
    "Ticket",
    "ExpectTicket",
    "CommitTicket",
    "StreamTicket",
    "dedup_plan",
    "dedup_rows",
    "expect_plan",
    "expect_bitmap",
    "commit_plan",
    "commit_seg_plan",
    "commit_programme",
    "Checkpoint",
    "CheckpointResult",
    "Commit",
    "CommitBatch",
    "DeviceLog",
    "PendingResults",
    "MirshaError",
    "MirshaUnavailable",
    "bucket_order",
    "HASHERS",
    "hasher_info",
    "order_plan",
    "device_count",
    "hash_batch_multi",
    "MultiEngine",
    "mismatch_indices",
    "eventlog",
    "hashdata",
    "sharding",
    "ActionResults",
    "Actions",
    "GpuHash",
    "HashRequest",
    "HashResult",
    "Processor",
    "ProcessorWorkPool",
    "gpu_hasher",
]
