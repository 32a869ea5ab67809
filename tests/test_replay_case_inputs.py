"""No GPU needed: what tests/test_gpu_replay_geometry.py rests on, checked on the CPU by the oracle alone.

  * every stored slot of every case, walked by a plain Python restatement of the reference's _compute_n_step over the
    oracle's arrays, equals ``ReplayOracle.gather`` in reward, gamma, nonterminal and next observation;
  * the rings reach what the cases are meant for: over the table, for every n_step > 1, walks that exhaust n_step, stop at
    a done, at a truncation and at an open link, follow a wrapping link, change stride mid-walk (the fused front launch's
    predictor misses), predict a slot outside [0, capacity), and end on the predicted slot (n_step = 2 follows one link, which
    is its own prediction: no stride change, no slot out of range there); the tree depths are exactly L = 1 .. 15;
  * the edge masses of the fused-front test: the clamp masses return size - 1 and the boundary masses land on both sides of
    a leaf boundary, on the oracle."""
import numpy as np
import pytest

from oracle import per_ref
from tests import replay_cases as R

STOPS = {"exhausted", "done", "truncated", "open"}
PREDICTOR = {"wrapping_link", "stride_change", "pred_out_of_range", "ends_on_pred"}


@pytest.mark.parametrize("name", list(R.CASES))
def test_gather_equals_the_plain_walk_on_every_stored_slot(name):
    orc, _ = R.build_ring(R.CASES[name])
    slots = np.arange(orc.length)
    g = orc.gather(slots)
    for s in slots:
        path, ret, gamma, _ = R.walk(orc, s)
        last = path[-1]
        fl = int(orc.flags[last])
        assert g["reward"][s] == np.float32(ret), s
        assert g["gamma"][s] == np.float32(gamma), s
        assert bool(g["nonterminal"][s]) == (not fl & per_ref.FLAG_DONE), s
        nxt = orc.succ_obs[last] if fl & per_ref.FLAG_HAS_NEXT else orc.obs[s]
        assert np.array_equal(g["next_obs"][s], nxt), s
    np.testing.assert_array_equal(g["obs"], orc.obs[:orc.length])
    np.testing.assert_array_equal(g["action"], orc.action[:orc.length])


@pytest.fixture(scope="module")
def classes():
    """case name -> the classes (R.classify) seen over every stored slot."""
    seen = {}
    for name, case in R.CASES.items():
        orc, _ = R.build_ring(case)
        seen[name] = set().union(*(R.classify(orc, s) for s in range(orc.length)))
    return seen


def test_every_walk_class_occurs_for_every_n_step(classes):
    by_n = {}
    for name, kinds in classes.items():
        by_n.setdefault(R.CASES[name].n_step, set()).update(kinds)
    assert set(by_n) == {1, 2, 3, 4, 8, 15}
    assert by_n[1] == {"exhausted"}                              # a one-step walk follows no link
    # n_step = 2 follows one link: the predicted slot idx + 1 * d IS that link -- always in range, and there is no second
    # stride to differ from the first.  Those two classes cannot occur there; everything else must, at every length.
    one_link = {"stride_change", "pred_out_of_range"}
    assert not by_n[2] & one_link
    for n_step, kinds in by_n.items():
        if n_step > 1:
            want = STOPS | PREDICTOR - (one_link if n_step == 2 else set())
            assert kinds >= want, (n_step, sorted(want - kinds))


def test_depths_fills_and_batches_are_the_ones_meant():
    levels = {R.tree_levels(c.capacity) for c in R.CASES.values()}
    assert levels == set(range(1, 16))
    assert {R.tree_levels(c.capacity) for c in R.EDGE_CASES.values()} == {6, 8, 14}
    for L, name in R.GRAPH_CASES.items():
        c = R.CASES[name]
        assert R.tree_levels(c.capacity) == L and c.rows_written >= c.capacity and c.use_per
    for cap in (8, 129, 1023, 8192):
        sizes = {min(c.rows_written, cap) for c in R.CASES.values() if c.capacity == cap}
        assert sizes >= {1, 2, cap // 2 + 1, cap - 1, cap}
    for cap in (127, 128, 2047):
        assert {c.B for c in R.CASES.values() if c.capacity == cap} >= {16, 256, 272, 512, 528}
    assert {c.C for c in R.CASES.values()} == {1, 4, 7, 10}
    assert {c.rows_written < c.capacity for c in R.CASES.values() if not c.use_per} == {True, False}
    assert 60 <= len(R.CASES) <= 80
    for c in list(R.CASES.values()) + list(R.EDGE_CASES.values()):
        assert c.B % 16 == 0 and 1 <= c.n_step <= 15


def test_wrapped_rings_hold_wrapping_links_strides_and_open_rows():
    """A ring written over: links that wrap, more than one stride where capacity % n_streams != 0, and rows with HAS_NEXT but
    no stored successor.  (Those are the streams' open rows.  Overwriting cannot detach a predecessor that is still stored:
    a predecessor is the older row of the two, so the round-robin writer reaches it first.)"""
    for name in ("depth_cap129", "nstep3_g0.99_s8_cap257", "nstep15_g0.5_s3_cap1000"):
        case = R.CASES[name]
        orc, _ = R.build_ring(case)
        fl = orc.flags
        open_rows = (fl & per_ref.FLAG_HAS_NEXT != 0) & (fl & per_ref.FLAG_TRUNC == 0) & (orc.link < 0)
        assert 0 < int(open_rows.sum()) <= case.n_streams, name
        assert int(((orc.link >= 0) & (orc.link < np.arange(orc.capacity))).sum()) > 0
        if case.capacity % case.n_streams:
            strides = {int(d) for d in (orc.link - np.arange(orc.capacity))[orc.link >= 0]}
            assert len(strides) > 1, name


@pytest.mark.parametrize("name", list(R.EDGE_CASES))
def test_edge_masses_clamp_and_straddle_leaf_boundaries(name):
    case = R.EDGE_CASES[name]
    orc, prio = R.build_ring(case)
    size = orc.length
    assert size == min(case.rows_written, case.capacity)
    mass, clamps, leaves = R.edge_masses(case, orc.sampler, size)
    idx, w, p_sum, p_min = orc.sampler.sample(size, mass)
    assert idx.min() >= 0 and idx.max() <= size - 1
    assert idx[0] == 0
    tree = orc.sampler.sum_tree
    for k in clamps:                                             # the descent itself ends behind the stored rows
        assert tree.scan_lower_bound(mass[k]) > size - 1 and idx[k] == size - 1
    assert len(leaves) == 4 and any(b == a + 1 for a, b in zip(leaves, leaves[1:]))
    for j, leaf in enumerate(leaves):
        lo, hi, at = idx[4 + 3 * j:7 + 3 * j]                     # last mass left of the boundary, first on it, the prefix sum
        assert lo == leaf - 1 and hi == leaf and at in (leaf - 1, leaf), (leaf, lo, hi, at)
