"""No GPU needed: the host half of the direct all-reduce tests (tests/test_gpu_direct_worlds.py).

1. The slices of ``slice_range`` partition the float4s for every world and length.
2. The inputs of tests/direct_cases.py make the summation order visible: from world 3 up the rank-ordered sum differs, by
   bit pattern, from the reversed-order sum and from the float64 sum rounded once -- in every non-empty slice and in every
   tail element.  Without this a kernel that sums in another order could pass the GPU tests by accident (at world 2 it does:
   two addends have one sum).
3. ``prism_direct_reduce_scatter`` / ``prism_direct_all_gather`` / ``prism_direct_phase`` refuse a bad descriptor before
   anything is launched."""
import ctypes
import os

import numpy as np
import pytest

from tests import direct_cases as C
from tests import direct_ref as R


@pytest.mark.parametrize("W", C.WORLDS)
def test_slices_partition_the_float4s(W):
    for n in sorted(set(range(1, 201)) | set(C.lengths(W)) | {C.CLAMP_CASE[1]}):
        at, seen_empty = 0, False
        for s in range(W):
            lo, hi = R.slice_range(n, W, s)
            assert lo == at and hi >= lo, (W, n, s)          # ordered, disjoint, no gap
            assert not (seen_empty and hi > lo), (W, n, s)   # empty slices only at the end
            seen_empty = seen_empty or hi == lo
            at = hi
        assert at == n >> 2, (W, n)
        # what the ranks reduce, tail included, covers every float exactly once
        fr = [R.float_range(n, W, s) for s in range(W)]
        assert fr[0][0] == 0 and fr[-1][1] == n and all(fr[s][1] == fr[s + 1][0] for s in range(W - 1)), (W, n)


def test_case_lengths_are_the_ones_meant():
    for W in C.WORLDS:
        ns = C.lengths(W)
        assert {1, 3, 4, 7, 4 * W, 4 * W + 5, 4 * 256 * W + 3, 4 * (256 * W + 1) + 1, 100_003} <= set(ns) and 0 not in ns
        if W > 1:
            lo, hi = R.slice_range(4 * W - 4, W, W - 1)
            assert hi == lo and R.slice_range(4 * W - 4, W, W - 2) == (W - 2, W - 1)       # only the last slice is empty
        n = 4 * 256 * W + 3
        assert all(R.slice_range(n, W, s) == (256 * s, 256 * s + 256) for s in range(W))   # one pass of one block each
    W, n = C.CLAMP_CASE
    lo, hi = R.slice_range(n, W, 0)
    assert hi - lo > 512 * 256 and n & 3 == 2                                               # the 512-block clamp binds


@pytest.mark.parametrize("W,n", [c for c in C.CASES + (C.CLAMP_CASE,) if c[0] >= 3], ids=lambda v: str(v))
def test_inputs_tell_the_summation_orders_apart(W, n):
    bufs, want = C.inputs(W, n)
    assert want.dtype == np.float32 and all(b.dtype == np.float32 and b.shape == (n,) for b in bufs)
    w = R.bits(want)
    for other in (R.reversed_sum(bufs), R.float64_sum(bufs)):
        diff = w != R.bits(other)
        for s in range(W):
            lo, hi = R.slice_range(n, W, s)
            if hi > lo:
                assert diff[4 * lo:4 * lo + 4].all() and diff[4 * hi - 4:4 * hi].all(), (W, n, s)    # both edges of the slice
        assert diff[R.tail_start(n):].all(), (W, n)                                                  # every tail element
    # the crafted elements are what the docstring of direct_cases says they are
    pos = C.crafted_positions(W, n)
    assert (want[pos] == C.BIG).all() and (R.reversed_sum(bufs)[pos] >= C.BIG + 2).all()
    # and the random rest depends on the order often enough to notice a slip anywhere else
    if n >= 1000:
        rest = np.ones(n, bool)
        rest[pos] = False
        assert (w != R.bits(R.reversed_sum(bufs)))[rest].mean() > 0.15


def test_iterated_reference_is_five_ordered_sums():
    bufs, want = C.inputs(3, 17)
    s = want
    for _ in range(4):
        s = R.ordered_sum([s, s, s])
    np.testing.assert_array_equal(R.bits(R.iterated(bufs, 5)), R.bits(s))
    for r in range(3):
        got = R.after_reduce_scatter(bufs, r)
        lo, hi = R.float_range(17, 3, r)
        keep = np.ones(17, bool)
        keep[lo:hi] = False
        assert (R.bits(got)[lo:hi] == R.bits(want)[lo:hi]).all() and (R.bits(got)[keep] == R.bits(bufs[r])[keep]).all()


# ---- refusals: every call below fails a check of direct.hip's fill() or the phase check, so no launch is reached ----------
@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from prism_amd import _native as N
    if not os.path.exists(N.LIB_PATH):
        g.build()
    return N.lib()


def _fake_desc(world=3, rank=1, n=1000):
    """A descriptor every check accepts, over buffers that do not exist (16-byte-aligned made-up addresses)."""
    from prism_amd import _native as N
    d = N.DirectDesc()
    d.world, d.rank, d.n, d.wait_seconds = world, rank, n, 0.2
    for s in range(N.MAX_PEERS):
        d.bufs[s], d.flags[s] = 0x10000000 + 0x100000 * s, 0x20000000 + 0x1000 * s
    return d


def _edit(**kw):
    def f(d):
        for k, v in kw.items():
            setattr(d, k, v)
    return f


def _item(field, s, v):
    def f(d):
        getattr(d, field)[s] = v
    return f


DESC_REFUSALS = [
    ("world 0", _edit(world=0, rank=0), b"world / rank out of range"),
    ("world 9", _edit(world=9), b"world / rank out of range"),
    ("rank = world", _edit(rank=3), b"world / rank out of range"),
    ("rank < 0", _edit(rank=-1), b"world / rank out of range"),
    ("n = 0", _edit(n=0), b"empty buffer"),
    ("n < 0", _edit(n=-4), b"empty buffer"),
    ("misaligned own buffer", _item("bufs", 1, 0x10100004), b"peer buffers must be mapped and 16-byte aligned"),
    ("misaligned peer buffer", _item("bufs", 2, 0x10200008), b"peer buffers must be mapped and 16-byte aligned"),
    ("unmapped peer buffer", _item("bufs", 0, None), b"peer buffers must be mapped and 16-byte aligned"),
    ("negative wait", _edit(wait_seconds=-1.0), b"wait_seconds out of range"),
    ("endless wait", _edit(wait_seconds=1e6), b"wait_seconds out of range"),
]


@pytest.mark.parametrize("entry", ["reduce_scatter", "all_gather", "phase"])
@pytest.mark.parametrize("case", range(len(DESC_REFUSALS)), ids=[c[0] for c in DESC_REFUSALS])
@pytest.mark.parametrize("use_flags", [0, 1])
def test_direct_refusals_without_device(lib, entry, case, use_flags):
    _, edit, text = DESC_REFUSALS[case]
    d = _fake_desc()
    edit(d)
    rc = {"reduce_scatter": lambda: lib.prism_direct_reduce_scatter(ctypes.byref(d), use_flags, None),
          "all_gather": lambda: lib.prism_direct_all_gather(ctypes.byref(d), use_flags, None),
          "phase": lambda: lib.prism_direct_phase(ctypes.byref(d), 1 + use_flags, 3, None)}[entry]()
    assert rc == -1, (rc, lib.prism_last_error())
    assert text in lib.prism_last_error(), lib.prism_last_error()


@pytest.mark.parametrize("entry", ["reduce_scatter", "all_gather", "phase"])
@pytest.mark.parametrize("missing", [0, 1, 2])
def test_direct_refuses_missing_flags(lib, entry, missing):
    d = _fake_desc()
    d.flags[missing] = None
    rc = {"reduce_scatter": lambda: lib.prism_direct_reduce_scatter(ctypes.byref(d), 1, None),
          "all_gather": lambda: lib.prism_direct_all_gather(ctypes.byref(d), 1, None),
          "phase": lambda: lib.prism_direct_phase(ctypes.byref(d), 1, 1, None)}[entry]()      # (the phase launch always needs them)
    assert rc == -1 and b"flag arrays missing" in lib.prism_last_error(), (rc, lib.prism_last_error())
    assert lib.prism_direct_reduce_scatter(None, 0, None) == -1 and b"null descriptor" in lib.prism_last_error()


@pytest.mark.parametrize("phase,what", [(0, 3), (4, 3), (-1, 1), (1, 0), (2, 4), (3, -1)])
def test_direct_phase_refuses_phase_and_what_out_of_range(lib, phase, what):
    d = _fake_desc()
    assert lib.prism_direct_phase(ctypes.byref(d), phase, what, None) == -1
    assert b"phase is 1..3, what is 1 (announce), 2 (wait) or 3" in lib.prism_last_error(), lib.prism_last_error()
