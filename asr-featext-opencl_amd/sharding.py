"""Utterance sharding across the GPUs of one node.

The path shards trivially: utterances are independent, so rank r of n takes utterances
r, r+n, r+2n, ... (round-robin, as BASELINE.json configs[3] states) and runs the ordinary batch
entry points on its own device.  There is no data-path collective; ``torch.distributed`` (RCCL on
GPUs, gloo in the CPU tests) is used only to agree on totals and timings.

The reference has no multi-device code at all: its "threads" loop runs the worker sequentially over
one file queue (ASR_OCL.cpp:340-368).
"""
import numpy as np


def shard_indices(n_utt, rank, world):
    """Indices of the utterances rank `rank` owns (round-robin)."""
    if not (0 <= rank < world):
        raise ValueError("rank out of range")
    return np.arange(rank, n_utt, world, dtype=np.int64)


def shard_layout(lengths, rank, world):
    """Pack this rank's utterances back to back: returns (indices, offsets, lengths, total_samples).
    Offsets are kept even so that the aligned 32-bit PCM load path applies."""
    lengths = np.asarray(lengths, dtype=np.int64)
    idx = shard_indices(lengths.size, rank, world)
    ln = lengths[idx]
    padded = ln + (ln & 1)
    off = np.zeros(idx.size, dtype=np.int64)
    if idx.size > 1:
        off[1:] = np.cumsum(padded[:-1])
    total = int(padded.sum())
    return idx, off, ln, total


def frames_of(lengths, window_size, shift):
    """Frames per utterance, integer arithmetic (parambase.cpp:16-19)."""
    lengths = np.asarray(lengths, dtype=np.int64)
    t = (lengths - (window_size - shift)) // shift
    return np.maximum(t, 0)


def gather_counts(local_frames, dist=None):
    """Sum of a per-rank frame count over all ranks (identity without torch.distributed)."""
    if dist is None or not dist.is_initialized():
        return int(local_frames)
    import torch
    t = torch.tensor([int(local_frames)], dtype=torch.int64)
    if dist.get_backend() == "nccl":
        t = t.cuda()
    dist.all_reduce(t, op=dist.ReduceOp.SUM)
    return int(t.item())


def max_over_ranks(value, dist=None):
    """Max of a per-rank scalar (the bench's step time) over all ranks."""
    if dist is None or not dist.is_initialized():
        return float(value)
    import torch
    t = torch.tensor([float(value)], dtype=torch.float64)
    if dist.get_backend() == "nccl":
        t = t.cuda()
    dist.all_reduce(t, op=dist.ReduceOp.MAX)
    return float(t.item())


def merge_speaker_acc(parts):
    """Sum of the per-speaker accumulators of several ranks (MfccHip.batch_speaker_stats of each rank's pooling pass):
    parts is a sequence of (count [n_spk] int64, acc [n_spk][4][Wn] float64) in ascending rank order; counts, S and S2
    are added and min / max taken in that order, starting from rank 0's values as they are.  Returns (count, acc): the
    prior of every rank's second pass (``batch_set_speakers(..., prior=(count, acc), mode=SPK_PRIOR_ONLY)``).  Utterances
    of one speaker may lie on different devices (shard_indices deals them round-robin): pass 1 pools per rank, the host
    merges, pass 2 normalises."""
    parts = list(parts)
    if not parts:
        raise ValueError("no accumulators to merge")
    count = np.array(parts[0][0], dtype=np.int64, copy=True)
    acc = np.array(parts[0][1], dtype=np.float64, copy=True)
    if acc.ndim != 3 or acc.shape[0] != count.size or acc.shape[1] != 4:
        raise ValueError("acc must be [n_spk][4][Wn]")
    for c, a in parts[1:]:
        c = np.asarray(c, dtype=np.int64)
        a = np.asarray(a, dtype=np.float64)
        if c.shape != count.shape or a.shape != acc.shape:
            raise ValueError("accumulators of different shapes")
        count += c
        acc[:, 0] += a[:, 0]
        acc[:, 1] += a[:, 1]
        acc[:, 2] = np.minimum(acc[:, 2], a[:, 2])
        acc[:, 3] = np.maximum(acc[:, 3], a[:, 3])
    return count, acc
