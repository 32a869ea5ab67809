"""GPU: every bulk install of ring contents (``load_arrays``, ``fill_replay``, ``load``) goes through one sealing step, so
  * a buffer that has been used ends in exactly the state a freshly constructed one ends in -- the ring arrays whole, the
    trees whole, every host mirror -- and goes on identically from there, and
  * on a fresh buffer the sealed state is what the formulas say: ``back`` the inverse of ``link``, the given leaves under
    the trees' own pairwise float32 sums, nothing beyond the rows."""
import weakref

import numpy as np
import pytest
import torch

from tests.test_gpu_ingest import FIELDS, Streams, _flat

pytestmark = pytest.mark.gpu

CAP, SHAPE = 13, (7,)                       # no power of two; 7 elements a row: the unaligned row copies


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return "cuda:0"


def _make(dev, use_per):
    from prism_amd.experience import HipReplayBuffer
    return HipReplayBuffer(CAP, 8, device=dev, n_step=3, gamma=0.99, use_per=use_per, seed=11)


def _chains(rng, n_rows, first_id=0):
    """n_rows Timesteps of two interleaved open chains (row i belongs to chain i % 2), and the two nodes still to come."""
    from prism_amd.experience import Timestep
    mk = lambda i: Timestep(id=first_id + i, obs=torch.from_numpy((rng.random(SHAPE) < 0.3).astype(np.float32)))
    steps = [mk(i) for i in range(n_rows + 2)]
    for i, t in enumerate(steps[:n_rows]):
        t.reward, t.action, t.done, t.truncated = float(rng.standard_normal()), int(rng.integers(0, 6)), False, False
        t.next = weakref.ref(steps[i + 2])
    return steps[:n_rows], steps[n_rows:]


def _batch_step(buf, r):
    return buf.extend_batch(r["obs"], r["next_obs"], r["action"], r["reward"], r["done"], r["trunc"])


def _dirty(dev, use_per):
    """A buffer that has wrapped, holds open rows of both producers, staged rows and a live pending predecessor."""
    rng = np.random.default_rng(1)
    buf = _make(dev, use_per)
    steps, tail = _chains(rng, 22)
    for i, t in enumerate(steps[:20]):                      # 20 rows into 13 slots (a flush carries at most 13)
        buf.extend(t)
        if i % 10 == 9:
            buf.flush()
    _batch_step(buf, Streams(rng, SHAPE).step(range(3), force_open=True))
    for t in steps[20:]:
        buf.extend(t)                                       # left unflushed
    assert buf._n_staged == 2 and buf._pending and len(buf) == CAP and int((buf._stream_tab >= 0).sum()) == 3
    return buf, (steps, tail)                               # (the Timesteps stay alive: _pending holds weak successors)


def _load_arrays(buf, _tmp):
    rng = np.random.default_rng(2)
    obs = (rng.random((5,) + SHAPE) < 0.3).astype(np.float32)
    link = np.array([1, -1, 4, -1, -1], np.int32)           # row 2 links into row 4, which is no stored item
    flags = np.where(link >= 0, 4, 1).astype(np.uint8)
    buf.load_arrays(obs, obs[np.maximum(link, 0)], rng.standard_normal(5).astype(np.float32),
                    rng.integers(0, 6, 5).astype(np.int32), flags, link,
                    priorities=torch.tensor([0.5, 2.0, 1.25, 0.75]), n_sampleable=4)
    return 5, 4, 4


def _fill_replay(buf, _tmp):
    from prism_amd.synthetic import fill_replay
    fill_replay(buf, 8, obs_shape=SHAPE, n_streams=2, seed=5)
    return 8, 8, 8


def _load_dir(buf, tmp):
    buf.load(tmp)
    return 9, 9, 9


LOADERS = {"load_arrays": _load_arrays, "fill_replay": _fill_replay, "load": _load_dir}


def _state(buf):
    torch.cuda.synchronize()
    st = {k: getattr(buf, k).cpu().numpy() for k in FIELDS + ("status",) if getattr(buf, k) is not None}
    st["host"] = (len(buf), buf.buffer._writer._cursor, buf._serial, buf._n_staged, dict(buf._pending), buf._valid_rows())
    st["slot_id"] = buf._slot_id.copy()
    return st


def _assert_equal_states(a, b):
    assert a.keys() == b.keys()
    for k in a:
        if k == "host":
            assert a[k] == b[k], (a[k], b[k])
        else:
            np.testing.assert_array_equal(a[k], b[k], err_msg=k)


@pytest.mark.parametrize("use_per", [True, False], ids=["per", "uniform"])
@pytest.mark.parametrize("loader", list(LOADERS))
def test_used_buffer_equals_fresh_after_bulk_install(dev, tmp_path, loader, use_per):
    if loader == "load":                                    # a directory saved from a third buffer: 9 rows, two chains
        src = _make(dev, use_per)
        for t in _chains(np.random.default_rng(3), 9, first_id=500)[0]:
            src.extend(t)
        src.save(str(tmp_path))
    used, keep = _dirty(dev, use_per)
    fresh = _make(dev, use_per)
    for buf in (used, fresh):
        rows, size, cursor = LOADERS[loader](buf, str(tmp_path))
        assert (len(buf), buf.buffer._writer._cursor, buf._serial) == (size, cursor, cursor)
        assert buf._pending == {} and buf._n_staged == 0 and buf._valid_rows() == rows
        assert (buf._slot_id[rows:] == -1).all() and (buf._slot_id[:rows] != -1).all()
        assert buf._stream_tab is None or int((buf._stream_tab != -1).sum()) == 0
        assert int(buf.status.item()) == 0
    assert used._stream_tab is not None and fresh._stream_tab is None
    _assert_equal_states(_state(used), _state(fresh))
    # both go on identically: 6 steps of 3 streams wrap the ring again, then one sample() from equal seeds and draw counts
    gen = Streams(np.random.default_rng(4), SHAPE)
    for r in [gen.step(range(3)) for _ in range(6)]:
        assert _batch_step(used, r) == _batch_step(fresh, r)
    _assert_equal_states(_state(used), _state(fresh))
    assert used.seed == fresh.seed and used._draws + used._fused_draws == fresh._draws + fresh._fused_draws == 0
    got = []
    for buf in (used, fresh):
        batch, info = buf.sample(return_info=True)
        torch.cuda.synchronize()
        got.append({k: v.clone() for k, v in {**_flat(batch), **info}.items()})
    assert got[0].keys() == got[1].keys() and ("_weight" in got[0]) == use_per
    for k in got[0]:
        assert torch.equal(got[0][k], got[1][k]), k


def test_fill_replay_on_a_fresh_buffer_is_sealed_by_the_formulas(dev):
    """``fill_replay`` of a whole fresh ring, against the fill's draw order restated here and the oracle's segment tree."""
    from oracle import per_ref
    from prism_amd.synthetic import fill_replay
    buf = fill_replay(_make(dev, True), CAP, obs_shape=SHAPE, n_streams=2, seed=5)
    n, O, tc = CAP, int(np.prod(SHAPE)), buf.tree_capacity
    gen = torch.Generator(device=dev)
    gen.manual_seed(5)
    done = (torch.rand(n, device=dev, generator=gen) < 0.017).cpu().numpy()
    for _ in range(2):                                      # observations, then the open chains' successors
        torch.rand(n, O, device=dev, generator=gen)
    torch.randn(n, device=dev, generator=gen)               # reward
    torch.randint(0, 6, (n,), device=dev, generator=gen, dtype=torch.int32)
    prio = (torch.randn(n, device=dev, generator=gen).abs().pow(0.5) + 1e-8).cpu().numpy()
    link, back, tree = buf.link.cpu().numpy(), buf.back.cpu().numpy(), buf.tree.cpu().numpy()
    want_link = np.where((np.arange(n) + 2 < n) & ~done, np.arange(n) + 2, -1)
    np.testing.assert_array_equal(link, want_link)
    want_back = np.full(n, -1)
    want_back[want_link[want_link >= 0]] = np.flatnonzero(want_link >= 0)          # the inverse of link
    np.testing.assert_array_equal(back, want_back)
    assert (want_link >= 0).any()
    np.testing.assert_array_equal(tree[tc:tc + n, 0], prio)
    np.testing.assert_array_equal(tree[tc:tc + n, 1], prio)
    assert (tree[tc + n:, 0] == 0.0).all() and (tree[tc + n:, 1] == np.finfo(np.float32).max).all()
    ref = per_ref.SegmentTree(CAP, False)                   # float32 pairwise sums, node = left + right
    assert ref.capacity == tc
    ref.update(np.arange(n), prio)
    assert tree[1, 0] == ref.values()[1] and tree[1, 1] == prio.min()
    np.testing.assert_array_equal(tree[1:, 0], ref.values()[1:])
    assert buf.per_state.cpu().tolist() == [1.0, 0.0, 0.0, 0.0] and len(buf) == CAP and buf.buffer._writer._cursor == 0
