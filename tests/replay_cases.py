"""Replay geometries and chain shapes as a case table, shared by tests/test_gpu_replay_geometry.py (the kernels against the
oracle, bit for bit) and tests/test_replay_case_inputs.py (the cases shown on the CPU, by the oracle alone, to reach the
branches they are meant for).  numpy only.

A case is everything that fixes its ring: (capacity, rows_written, n_streams, n_step, gamma, C, B, use_per, seed).  The ring
is what ``ReplayOracle.insert`` leaves after `rows_written` rows of `n_streams` interleaved environment streams (about 7 % of
the rows end an episode, 3 % are truncations), fed row by row with each stream's previous slot.  rows_written < capacity is a
partial fill; rows_written > capacity a ring written over: links that wrap (link < slot) and a stride that changes across
the wrap when capacity % n_streams != 0.  Rows with HAS_NEXT and link -1 are the streams' open rows (the successor is not
stored yet): overwriting cannot detach a predecessor that is still stored, because the predecessor is the older row of the
two and the round-robin writer reaches it first.

Every axis varies around one base case (n_streams 3, n_step 3, gamma 0.99, C 4, B 16, prioritized), not as a product:
  depth    capacities that give L = log2(tree_capacity) = 1 .. 15 at least once, 2^k - 1 and 2^k on both sides of L = 7 (the
           register-top loop of the fused descent) and L = 8 (dense writeback), every trip length 1 .. 6 below the seven
           register levels (L = 8 .. 13) and two trips (L = 14, 15)
  fill     1, 2, cap / 2 + 1, cap - 1 rows of cap (the partial-fill query's closed form)
  batch    16, 256 | 272 (split writeback), 512 | 528 (one and two passes)
  nstep    n_step 1, 2, 3, 4, 8, 15 x gamma 0.99, 1.0, 0.5 x 1, 3, 8 streams, on rings written 2 - 3 times over
  chan     C = 1, 7, 10 (O / 4 = 25, 175, 250 of the front launch's 256 threads copy a row)
  uniform  uniform replay at a partial and a full ring"""
import collections
import functools

import numpy as np

from oracle import per_ref

Case = collections.namedtuple("Case", "capacity rows_written n_streams n_step gamma C B use_per seed")

P_DONE, P_TRUNC = 0.07, 0.03


def _case(capacity, rows_written=None, n_streams=3, n_step=3, gamma=0.99, C=4, B=16, use_per=True, seed=0):
    return Case(capacity, capacity if rows_written is None else rows_written, n_streams, n_step, gamma, C, B, use_per, seed)


def _wrapped(cap):
    """Rows that take the writer once round and a third of the way again: wrapping links at every depth."""
    return cap + cap // 3 + 5


CASES = {}
DEPTH_CAPACITIES = (1, 2, 3, 7, 8, 31, 32, 63, 64, 127, 128, 129, 255, 256, 511, 1023, 2047, 4095, 8191, 8192, 16383, 32767)
for _i, _cap in enumerate(DEPTH_CAPACITIES):
    CASES[f"depth_cap{_cap}"] = _case(_cap, _wrapped(_cap), seed=100 + _i)
for _cap in (8, 129, 1023, 8192):
    for _size in (1, 2, _cap // 2 + 1, _cap - 1):
        CASES[f"fill_cap{_cap}_size{_size}"] = _case(_cap, _size, seed=200 + _size % 97)
for _cap in (127, 128, 2047):
    for _B in (16, 256, 272, 512, 528):
        CASES[f"batch_cap{_cap}_b{_B}"] = _case(_cap, _wrapped(_cap), B=_B, seed=300 + _B)
# n-step: every n_step meets every gamma and every stream count (a Latin square, not the product), on both capacities
_GAMMAS, _STREAMS = (0.99, 1.0, 0.5), (1, 3, 8)
for _i, _n in enumerate((1, 2, 3, 4, 8, 15)):
    for _j in range(3):
        _cap = (257, 1000)[(_i + _j) % 2]
        _g, _s = _GAMMAS[_j], _STREAMS[(_i + _j) % 3]
        CASES[f"nstep{_n}_g{_g}_s{_s}_cap{_cap}"] = _case(_cap, 2 * _cap + _cap // 2 + 3, n_streams=_s, n_step=_n, gamma=_g,
                                                         seed=400 + 3 * _i + _j)
for _C in (1, 7, 10):
    CASES[f"chan_c{_C}"] = _case(1023, _wrapped(1023), C=_C, seed=500 + _C)
CASES["uniform_partial"] = _case(1000, 700, use_per=False, seed=600)
CASES["uniform_full"] = _case(1000, 2300, use_per=False, seed=601)

# full rings that run a fourth fused step, so that the third and the fourth come from the captured graph: one per L
GRAPH_CASES = {6: "depth_cap63", 7: "depth_cap127", 8: "depth_cap255", 13: "depth_cap8191", 15: "depth_cap32767"}
# the fused front launch with given masses (clamps, leaf boundaries): partial and full rings of L = 6, 8, 14 at B = 16 and 272
EDGE_CASES = {}
for _cap, _L in ((63, 6), (255, 8), (16383, 14)):
    for _B in (16, 272):
        EDGE_CASES[f"edge_L{_L}_full_b{_B}"] = _case(_cap, _wrapped(_cap), B=_B, seed=700 + _L + _B)
        EDGE_CASES[f"edge_L{_L}_partial_b{_B}"] = _case(_cap, _cap // 2 + 1, B=_B, seed=720 + _L + _B)


def tree_levels(capacity):
    """L = log2(tree_capacity); tree_capacity is the power of two strictly greater than the capacity."""
    return int(capacity).bit_length()


def fused_steps(name):
    return 4 if name in GRAPH_CASES.values() else 3


@functools.lru_cache(maxsize=8)
def build_ring(case):
    """The oracle's ring of a case (treat as read-only: tests that write priorities take ``fresh_sampler``): rows fed to
    ``ReplayOracle.insert`` one by one, then every stored leaf set to sqrt(|N(0, 1)| + 1e-8) as fp32.  Returns
    (oracle, priorities of the stored slots)."""
    rng = np.random.default_rng(case.seed)
    O = 100 * case.C
    # (no sampler while the rows go in: every stored leaf is set below, the default priorities would be written for nothing)
    orc = per_ref.ReplayOracle(case.capacity, O, case.n_step, case.gamma, use_per=False)
    frame = lambda: (rng.random(O) < 0.1).astype(np.float32)
    cur = [frame() for _ in range(case.n_streams)]
    prev = [(-1, 0)] * case.n_streams                   # (slot, serial) of each stream's open row
    for serial in range(case.rows_written):
        e = serial % case.n_streams
        u = rng.random()
        done, trunc = u < P_DONE, P_DONE <= u < P_DONE + P_TRUNC
        nxt = frame()
        succ = None if done else (frame() if trunc else nxt)
        slot, at = prev[e]
        # (a ring smaller than the number of streams: the stream's open row was itself overwritten before its successor
        # came -- the slot now holds another stream's row, there is nothing to link)
        if slot >= 0 and serial - at >= case.capacity:
            slot = -1
        s = orc.insert(cur[e], succ, np.float32(rng.standard_normal()), int(rng.integers(0, 6)), done, trunc, not done, slot)
        prev[e] = (-1, 0) if done or trunc else (s, serial)
        cur[e] = nxt
    prio = np.sqrt(np.abs(rng.standard_normal(orc.length)).astype(np.float32) + np.float32(1e-8)).astype(np.float32)
    if case.use_per:
        orc.sampler = fresh_sampler(case, prio)
    return orc, prio


def set_priorities(sampler, prio):
    """Both trees as a bulk load of these leaves leaves them (HipReplayBuffer.load_arrays ``priorities=``)."""
    sampler.sum_tree.values()[:] = 0.0
    sampler.min_tree.values()[:] = np.finfo(np.float32).max
    idx = np.arange(prio.size)
    sampler.sum_tree.update(idx, prio)
    sampler.min_tree.update(idx, prio)
    sampler.max_priority = 1.0


def fresh_sampler(case, prio):
    """A sampler of the case's own (alpha = beta = 0.5) holding `prio`: what a test may write to."""
    smp = per_ref.PrioritizedSamplerOracle(case.capacity, 0.5, 0.5)
    set_priorities(smp, prio)
    return smp


# ---------------------------------------------------------------------------------------------- the walk, restated
def walk(orc, slot):
    """_compute_n_step (timestep_buffer.py:198-238) over the oracle's arrays in plain Python: (slots visited, return as
    float64, gamma ** rewards summed, why it stopped: 'exhausted' | 'done' | 'truncated' | 'open')."""
    F = per_ref
    cur, path, ret = int(slot), [int(slot)], 0.0
    for i in range(orc.n_step):
        ret += float(orc.reward[cur]) * float(orc.gammas[i])
        gamma = float(orc.gammas[i + 1])
        fl, nx = int(orc.flags[cur]), int(orc.link[cur])
        if (fl & F.FLAG_HAS_NEXT) and not (fl & F.FLAG_TRUNC) and i != orc.n_step - 1 and nx >= 0:
            cur = nx
            path.append(cur)
        else:
            break
    fl = int(orc.flags[cur])
    why = "exhausted" if len(path) == orc.n_step else "done" if fl & F.FLAG_DONE else \
        "truncated" if fl & F.FLAG_TRUNC else "open"
    return path, ret, gamma, why


def classify(orc, slot):
    """The classes of one walk as the fused front launch sees it (step_kernels.h step_front_kernel): how it stopped, and
    what became of the prediction idx + (n_step - 1) * d from the first link's stride d."""
    path, _, _, why = walk(orc, slot)
    kinds = {why}
    if len(path) > 1:
        d = path[1] - path[0]
        pred = path[0] + (orc.n_step - 1) * d
        if any(b < a for a, b in zip(path, path[1:])):
            kinds.add("wrapping_link")
        if any(b - a != d for a, b in zip(path, path[1:])):
            kinds.add("stride_change")
        if not 0 <= pred < orc.capacity:
            kinds.add("pred_out_of_range")
        elif path[-1] == pred:
            kinds.add("ends_on_pred")
    return kinds


# ---------------------------------------------------------------------------------------------- edge masses
def prefix_mass(sum_tree, leaf):
    """The fp32 mass at which the descent (SumSegmentTree scan_lower_bound: subtract as it goes, right when v > left) turns
    from leaf - 1 to `leaf`: the sum of the left siblings along the root-to-leaf path, added top down in fp32 -- the order in
    which the descent subtracts them.  Where a partial sum rounds, it lies a few units in the last place beside the boundary
    (``boundary_mass`` finds the boundary itself)."""
    v, cap = sum_tree.values(), sum_tree.capacity
    node, acc = int(leaf) + cap, []
    while node > 1:
        if node & 1:
            acc.append(v[node - 1])
        node >>= 1
    total = np.float32(0)
    for x in reversed(acc):
        total = np.float32(total + x)
    return total


def boundary_mass(sum_tree, leaf):
    """The largest fp32 mass whose descent ends left of `leaf` (the next float ends on it or right of it): bisection over the
    bit patterns of the non-negative floats on the oracle's own descent, which is monotone in the mass."""
    lo, hi = 0, int(np.float32(sum_tree.values()[1]).view(np.int32))          # scan(0) = 0 < leaf; scan(root) >= leaf or clamps
    as_f = lambda i: np.int32(i).view(np.float32)
    if sum_tree.scan_lower_bound(as_f(hi)) < leaf:
        return as_f(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if sum_tree.scan_lower_bound(as_f(mid)) < leaf:
            lo = mid
        else:
            hi = mid
    return as_f(lo)


def edge_masses(case, sampler, size):
    """B masses for the fused front launch: 0, p_sum, the float behind p_sum, 3e38; for four leaves (two of them neighbours:
    both boundaries of one leaf) the last mass left of the leaf's left boundary, the first one on it and the fp32 prefix sum
    there; the rest random in [0, p_sum).  Returns (masses, positions of the masses that must clamp, the leaves)."""
    rng = np.random.default_rng(case.seed + 7)
    p_sum = np.float32(sampler.sum_tree.query(0, size))
    mass = rng.uniform(0.0, float(p_sum), case.B).astype(np.float32)
    mass[:4] = [0.0, p_sum, np.nextafter(p_sum, np.float32(np.inf)), np.float32(3e38)]
    leaves = sorted({int(x) for x in (1, size // 3, size // 3 + 1, size - 1) if 0 < x < size})[:4]
    for j, leaf in enumerate(leaves):
        m = boundary_mass(sampler.sum_tree, leaf)
        mass[4 + 3 * j:7 + 3 * j] = [m, np.nextafter(m, np.float32(np.inf)), prefix_mass(sampler.sum_tree, leaf)]
    return mass, (2, 3), leaves
