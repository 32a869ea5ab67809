"""Host restatement of the direct all-reduce (prism_amd/csrc/direct.hip): which float4s rank s owns, and THE sum -- plain
float32 adds in rank order 0, 1, ..., W - 1, which is what the reduce-scatter kernel does to every element (vector lanes and
tail alike), so the comparison with the device is by bit pattern, without a tolerance.  The two other orders below are what a
kernel that lost the promise of include/prism_hip.h ("sum over s = 0..world-1 (in that order)") would most likely compute:
tests/test_direct_host.py proves on the host that the inputs of tests/direct_cases.py tell all three apart."""
import numpy as np


def slice_range(n, world, s):
    """float4 range [lo, hi) of slice s of n floats; the n & 3 trailing floats belong to the last rank."""
    n4 = n >> 2
    per = (n4 + world - 1) // world
    return min(per * s, n4), min(per * (s + 1), n4)


def float_range(n, world, s):
    """The floats rank s reduces: its float4s, and for the last rank the tail."""
    lo, hi = slice_range(n, world, s)
    return 4 * lo, (n if s == world - 1 else 4 * hi)


def tail_start(n):
    return (n >> 2) << 2


def ordered_sum(bufs):
    acc = np.asarray(bufs[0], dtype=np.float32).copy()
    for s in range(1, len(bufs)):
        acc = (acc + bufs[s]).astype(np.float32)
    return acc


def reversed_sum(bufs):
    return ordered_sum(list(bufs)[::-1])


def float64_sum(bufs):
    return np.sum(np.stack([np.asarray(b, dtype=np.float64) for b in bufs]), axis=0).astype(np.float32)


def iterated(bufs, rounds):
    """What every rank holds after `rounds` all-reduces in a row (each sums the W copies of the one before)."""
    out = None
    for _ in range(rounds):
        out = ordered_sum(bufs)
        bufs = [out] * len(bufs)
    return out


def after_reduce_scatter(bufs, r):
    """Buffer r once EVERY rank has run its reduce-scatter: the sum on what r owns, its own values everywhere else."""
    n, world = bufs[0].shape[0], len(bufs)
    out = np.asarray(bufs[r], dtype=np.float32).copy()
    lo, hi = float_range(n, world, r)
    out[lo:hi] = ordered_sum([b[lo:hi] for b in bufs])
    return out


def bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
