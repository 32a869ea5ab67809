"""The case table of the direct all-reduce tests: world sizes, lengths and inputs on which the summation ORDER shows.

Lengths per world W (``lengths(W)``): 1 and 3 (tail only, no float4); 4 and 7 (one float4: every slice but the first is
empty); 4 W - 4 (only the last slice empty); 4 W and 4 W + 5 (one float4 each, with and without a tail); 4 * 256 * W + 3
(every slice exactly one pass of one block); 4 (256 W + 1) + 1 (a second block in all slices but the last, which is one
float4 short of full); 100 003 (many blocks, no relation to W).  ``CLAMP_CASE``: at W = 3 a slice of more than 512 * 256
float4s, so the 512-block grid takes a second grid-stride trip.

Inputs (``inputs(W, n)``): seeded normals scaled by 10^k, k in -3..3 drawn per rank and element, so most sums depend on the
order of their addends; and CRAFTED elements, where rank 0 holds 2^24 and every other rank 1: in rank order every add is a
tie that rounds back to 2^24, any order that adds two of the ones first ends at 2^24 + 2 or beyond.  They sit in the first
and the last float4 of every non-empty slice and in every tail element -- the places an indexing slip moves."""
import functools

import numpy as np

from tests import direct_ref as R

WORLDS = tuple(range(1, 9))
CLAMP_CASE = (3, 4 * (3 * 512 * 256 + 17) + 2)
BIG, ONE = np.float32(2.0 ** 24), np.float32(1.0)


def lengths(W):
    ns = [1, 3, 4, 7, 4 * W - 4, 4 * W, 4 * W + 5, 4 * 256 * W + 3, 4 * (256 * W + 1) + 1, 100_003]
    return tuple(sorted({n for n in ns if n > 0}))


CASES = tuple((W, n) for W in WORLDS for n in lengths(W))


def crafted_positions(W, n):
    """Float indices of the crafted elements."""
    pos = set(range(R.tail_start(n), n))
    for s in range(W):
        lo, hi = R.slice_range(n, W, s)
        if hi > lo:
            pos.update(range(4 * lo, 4 * lo + 4))
            pos.update(range(4 * hi - 4, 4 * hi))
    return np.array(sorted(pos), dtype=np.int64)


@functools.lru_cache(maxsize=None)
def inputs(W, n):
    """(the W ranks' buffers, ordered_sum of them), float32, read-only: computed once and shared."""
    rng = np.random.default_rng(1000 * W + n % 997)
    bufs = (rng.standard_normal((W, n)) * 10.0 ** rng.integers(-3, 4, size=(W, n))).astype(np.float32)
    pos = crafted_positions(W, n)
    bufs[0, pos] = BIG
    bufs[1:, pos] = ONE
    bufs = tuple(bufs[s] for s in range(W))
    want = R.ordered_sum(bufs)
    for a in bufs + (want,):
        a.setflags(write=False)
    return bufs, want


def launch_order(W, salt=0):
    """A fixed scramble of the ranks: the order the one stream runs them in must not matter."""
    return [int(r) for r in np.random.default_rng(17 * W + salt).permutation(W)]
