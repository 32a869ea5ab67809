"""GPU: vectorised replay ingestion -- ``HipReplayBuffer.extend_batch`` / ``prism_replay_ingest``, one launch per step of N
environment streams.  The bar is bit-for-bit equality of the whole ring state (obs, succ_obs, reward, action, flags, link,
back, both trees whole, per_state) with
  * a twin ``HipReplayBuffer`` fed the same transitions as linked ``Timestep`` chains through ``extend()``, and
  * ``ReplayOracle.insert`` applied row by row by a host that tracks the owner of every slot (for the fields it holds)."""
import contextlib
import io
import weakref

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

FIELDS = ("obs", "succ_obs", "reward", "action", "flags", "link", "back", "tree", "per_state")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return "cuda:0"


class Streams:
    """Seeded transitions of environment streams: boolean observations (MinAtar's), an open stream's observation is the
    previous step's next observation."""

    def __init__(self, rng, obs_shape, p_done=0.07, p_trunc=0.03):
        self.rng, self.shape, self.p_done, self.p_trunc = rng, tuple(obs_shape), p_done, p_trunc
        self.carry = {}

    def _obs(self):
        return (self.rng.random(self.shape) < 0.3).astype(np.float32)

    def step(self, ids, force_open=False):
        n, rng = len(ids), self.rng
        obs = np.stack([self.carry.pop(e, None) if e in self.carry else self._obs() for e in ids])
        nxt = np.stack([self._obs() for _ in ids])
        done = rng.random(n) < self.p_done
        trunc = rng.random(n) < self.p_trunc            # (both at once happens too: DONE | TRUNC | HAS_NEXT)
        if force_open:
            done[:], trunc[:] = False, False
        for i, e in enumerate(ids):
            if not done[i] and not trunc[i]:
                self.carry[e] = nxt[i]
        return dict(ids=list(ids), obs=obs, next_obs=nxt, action=rng.integers(0, 6, n).astype(np.int32),
                    reward=rng.standard_normal(n).astype(np.float32), done=done, trunc=trunc)


class Trio:
    """The buffer under test, its extend()-fed twin and the row-by-row oracle, fed the same transitions."""

    def __init__(self, dev, capacity, obs_shape, use_per=True, oracle=True, n_step=3):
        from oracle import per_ref
        from prism_amd.experience import HipReplayBuffer
        mk = lambda: HipReplayBuffer(capacity, 8, device=dev, n_step=n_step, gamma=0.99, use_per=use_per, seed=11)
        self.dev, self.cap, self.O = dev, capacity, int(np.prod(obs_shape))
        self.buf, self.twin = mk(), mk()
        self.per_ref, self.use_per, self.n_step, self.with_oracle = per_ref, use_per, n_step, oracle
        self.ts_ids = iter(range(10 ** 9))
        self.reset_tracking()
        self.straddled = False

    def reset_tracking(self):
        self.orc = self.per_ref.ReplayOracle(self.cap, self.O, self.n_step, 0.99, use_per=self.use_per) \
            if self.with_oracle else None
        self.owner = np.full(self.cap, -1, np.int64)
        self.pending, self.cur, self.rows = {}, {}, 0

    def _timesteps(self, r):
        from prism_amd.experience import Timestep
        out = []
        for i, e in enumerate(r["ids"]):
            t = self.cur.pop(e, None) or Timestep(id=next(self.ts_ids))
            t.obs = torch.from_numpy(r["obs"][i])
            t.reward, t.action = float(r["reward"][i]), int(r["action"][i])
            t.done, t.truncated = bool(r["done"][i]), bool(r["trunc"][i])
            nxt = Timestep(id=next(self.ts_ids), obs=torch.from_numpy(r["next_obs"][i]))
            if t.truncated:
                t.next = nxt                             # a strong truncation node (timestep.py: next of a truncated step)
            elif not t.done:
                t.next = weakref.ref(nxt)
                self.cur[e] = nxt
            out.append(t)
        return out

    def feed(self, r, via="batch", place="host", obs_mode="f32", pass_ids=True):
        n, dev = len(r["ids"]), self.dev
        ts = self._timesteps(r)
        first = self.buf.buffer._writer._cursor
        self.straddled |= first + n > self.cap
        if via == "batch":
            cast = {"f32": np.float32, "u8": np.uint8, "bool": np.bool_}[obs_mode]
            a = dict(obs=r["obs"].astype(cast), next_obs=r["next_obs"].astype(cast), action=r["action"], reward=r["reward"],
                     done=r["done"], truncated=r["trunc"])
            ids = np.asarray(r["ids"], np.int64) if pass_ids else None
            if place != "host":                          # action int64 as Agent.forward returns it, flags as torch.bool
                a = {k: torch.from_numpy(v).to(dev) for k, v in a.items()}
                if place == "device_unaligned":
                    for k in ("obs", "next_obs"):
                        flat = torch.zeros(a[k].numel() + 1, dtype=a[k].dtype, device=dev)
                        flat[1:] = a[k].reshape(-1)
                        a[k] = flat[1:].view(a[k].shape)
                        assert a[k].data_ptr() % 4 != 0 or (a[k].dtype == torch.float32 and a[k].data_ptr() % 16 != 0)
                a["action"] = a["action"].long()
                ids = None if ids is None else torch.from_numpy(ids).to(dev)
            assert self.buf.extend_batch(stream_ids=ids, **a) == first
        else:
            for t in ts:
                self.buf.extend(t)
        for t in ts:
            self.twin.extend(t)
        self.twin.flush()
        for i, e in enumerate(r["ids"]):                 # the oracle's host: an owner per slot, a pending row per stream
            slot = self.rows % self.cap
            self.owner[slot] = self.rows
            rec = self.pending.pop(e, None)
            prev = rec[0] if rec is not None and self.owner[rec[0]] == rec[1] else -1
            done, trunc = bool(r["done"][i]), bool(r["trunc"][i])
            has_next = trunc or not done
            if self.orc is not None:
                so = self.orc.insert(r["obs"][i], r["next_obs"][i] if has_next else None, r["reward"][i], r["action"][i],
                                     done, trunc, has_next, prev)
                assert so == slot
            if not done and not trunc:
                self.pending[e] = (slot, self.rows)
            self.rows += 1
        return first

    def bump(self, rng, B=8):
        """A priority writeback, so that the running maximum (and with it the default priority) moves."""
        if not self.use_per:
            return
        self.buf.flush()
        idx = rng.integers(0, len(self.buf), B)
        td = (rng.random(B) * 4).astype(np.float32)
        for b in (self.buf, self.twin):
            b.update_priority(torch.from_numpy(idx).to(self.dev), torch.from_numpy(td).to(self.dev))
        if self.orc is not None:
            self.orc.sampler.update_priority(idx, td)

    def state(self, b):
        b.flush()
        torch.cuda.synchronize()
        return {k: getattr(b, k).cpu().numpy() for k in FIELDS if getattr(b, k) is not None}

    def check(self):
        got, want = self.state(self.buf), self.state(self.twin)
        assert got.keys() == want.keys()
        for k in got:
            np.testing.assert_array_equal(got[k], want[k], err_msg=k)
        assert len(self.buf) == len(self.twin) == min(self.rows, self.cap)
        assert self.buf.buffer._writer._cursor == self.twin.buffer._writer._cursor == self.rows % self.cap
        assert int(self.buf.status.item()) == 0
        o = self.orc
        if o is not None:
            for k in ("obs", "succ_obs", "reward", "action", "flags", "link"):
                np.testing.assert_array_equal(got[k], getattr(o, k), err_msg="oracle " + k)
            if self.use_per:
                np.testing.assert_array_equal(got["tree"][:, 0], o.sampler.sum_tree.values())
                np.testing.assert_array_equal(got["tree"][1:, 1], o.sampler.min_tree.values()[1:])
                assert got["per_state"][0] == np.float32(o.sampler.max_priority)
        return got


def _lockstep(dev, capacity, n, steps, seed, obs_shape=(10, 10, 4), use_per=True, **feed_kw):
    rng = np.random.default_rng(seed)
    trio, gen = Trio(dev, capacity, obs_shape, use_per=use_per), Streams(rng, obs_shape)
    for k in range(steps):
        trio.feed(gen.step(range(n)), **feed_kw)
        if k % 17 == 16:
            trio.bump(rng)
    return trio, trio.check()


@pytest.mark.parametrize("capacity,n,steps", [(37, 5, 60), (64, 3, 200), (257, 4, 400)])
def test_lockstep_streams_wrap_a_small_ring(dev, capacity, n, steps):
    """N streams in lockstep, identity stream ids, episode ends ~0.07 and truncations ~0.03, wrapping the ring many times;
    37 is no multiple of 5, so calls straddle the end of the ring."""
    trio, st = _lockstep(dev, capacity, n, steps, seed=capacity, pass_ids=False)
    assert (st["link"] >= 0).sum() > capacity // 2 and (st["flags"] & 1).any()
    if capacity == 37:
        assert trio.straddled


@pytest.mark.parametrize("capacity,n,steps", [(33, 33, 3), (5, 1, 23), (2100, 1030, 3)])
def test_whole_ring_single_stream_and_more_than_one_tree_pass(dev, capacity, n, steps):
    """n = capacity in one call (every row overwrites its own predecessor: all unlinked); N = 1; 1030 rows -- just above
    two 512-leaf passes of the tree writer and above the 1024-thread workgroup -- into a ring of 2100 (the third call wraps)."""
    trio, st = _lockstep(dev, capacity, n, steps, seed=n, pass_ids=False)
    if n == capacity:
        assert (st["link"] == -1).all() and (st["back"] == -1).all()
    else:
        assert (st["link"] >= 0).any()


def test_predecessor_overwritten_later_in_the_same_call(dev):
    """capacity 7, N = 5: the predecessor of row e (5 writes back) lies 2 slots ahead, so rows e + 2 of the same call
    overwrite it -- the plan workgroup must fall back to the sequential loop and leave its final state."""
    trio, st = _lockstep(dev, 7, 5, 40, seed=7, pass_ids=False)
    gen = Streams(np.random.default_rng(1), (10, 10, 4))
    for _ in range(3):
        trio.feed(gen.step(range(5), force_open=True), pass_ids=False)      # every row linked, three of five hit the case
    trio.check()


def test_stream_absent_for_a_whole_ring_returns_unlinked(dev):
    """Stream 0 leaves an open row, the others write `capacity` rows or more, stream 0 returns: its table entry is older
    than the ring, the slot it names belongs to another row, and the new row must start unlinked.  Boundary: absent for
    exactly capacity - 1 writes still links."""
    cap = 8
    rng = np.random.default_rng(5)
    trio, gen = Trio(dev, cap, (7,)), Streams(rng, (7,))
    trio.feed(gen.step([0, 1], force_open=True))                    # serials 0, 1
    trio.feed(gen.step([2, 3, 4, 5, 6, 7], force_open=True))        # 2 .. 7
    s = trio.feed(gen.step([0], force_open=True))                   # serial 8: 8 - 0 = capacity -> unlinked (slot 0 is its own)
    st = trio.check()
    assert s == 0 and st["back"][0] == -1 and st["link"][0] == -1
    trio.feed(gen.step([9, 10, 11, 12, 13, 14], force_open=True))   # 9 .. 14
    s = trio.feed(gen.step([0], force_open=True))                   # 15: 15 - 8 = 7 = capacity - 1 -> still linked
    st = trio.check()
    assert s == 7 and st["back"][7] == 0 and st["link"][0] == 7 and st["back"][0] == -1
    for _ in range(4):                                              # a long absence, many wraps
        trio.feed(gen.step([2, 3, 4, 5, 6], force_open=True))
    s = trio.feed(gen.step([1, 0], force_open=True))
    st = trio.check()
    assert st["back"][s] == -1 and st["back"][(s + 1) % cap] == -1


def test_explicit_ids_subsets_and_table_growth(dev):
    """Stream ids in non-identity order, a strict subset of the streams per call (absences of random length on a small
    ring), ids that make the table grow from 64 entries upwards while streams are open."""
    rng = np.random.default_rng(23)
    trio, gen = Trio(dev, 23, (10, 10, 4)), Streams(rng, (10, 10, 4))
    labels = [5, 0, 63, 2, 64, 999, 130, 4000]
    for k in range(150):
        pool = labels[:4] if k < 20 else labels
        ids = [int(e) for e in rng.permutation(pool)[:int(rng.integers(1, len(pool)))]]
        trio.feed(gen.step(ids))
        if k == 19:
            assert trio.buf._stream_tab.numel() == 64
        if k % 29 == 28:
            trio.bump(rng)
    st = trio.check()
    assert trio.buf._stream_tab.numel() == 4096 and (st["link"] >= 0).any()


@pytest.mark.parametrize("obs_mode,place", [("f32", "host"), ("u8", "host"), ("bool", "host"), ("f32", "device"),
                                            ("u8", "device"), ("bool", "device")])
@pytest.mark.parametrize("obs_shape", [(7,), (10, 10, 4)])
def test_observation_kinds_and_input_placement(dev, obs_shape, obs_mode, place):
    """float32 / uint8 / bool observations, host arrays through pinned staging and device tensors in place, with obs_elems a
    multiple of 4 (vector row copies) and not (7): every combination gives the twin's state, hence one another's."""
    _lockstep(dev, 11, 3, 25, seed=3, obs_shape=obs_shape, obs_mode=obs_mode, place=place)


@pytest.mark.parametrize("obs_mode", ["f32", "u8"])
def test_unaligned_device_views_take_the_scalar_copy(dev, obs_mode):
    """Device observations whose rows do not start on 16 (float32) / 4 (uint8) bytes: a view one element into a larger
    tensor, with obs_elems a multiple of 4."""
    _lockstep(dev, 11, 3, 12, seed=9, obs_shape=(8,), obs_mode=obs_mode, place="device_unaligned")


def test_uniform_replay(dev):
    trio, st = _lockstep(dev, 37, 5, 30, seed=2, use_per=False, pass_ids=False)
    assert "tree" not in st and (st["link"] >= 0).any()


def test_extend_and_extend_batch_interleaved(dev):
    """Timestep chains through extend() and vector steps through extend_batch() on ONE buffer: staged rows are flushed
    first (order kept), both advance the same serial, and a Timestep whose predecessor's slot an extend_batch row overwrote
    starts unlinked."""
    cap = 9
    rng = np.random.default_rng(4)
    trio, gen = Trio(dev, cap, (10, 10, 4)), Streams(rng, (10, 10, 4))
    s0 = trio.feed(gen.step([100], force_open=True), via="extend")          # chain 100: open row in slot 0, still staged
    trio.feed(gen.step([0, 1, 2, 3], force_open=True))                      # flushes it first
    trio.feed(gen.step([0, 1, 2, 3, 4], force_open=True))                   # slots 5 .. 8, 0: overwrites chain 100's row
    s1 = trio.feed(gen.step([100], force_open=True), via="extend")          # its successor: must not link to slot 0
    st = trio.check()
    assert s0 == 0 and s1 == 1 and st["back"][1] == -1 and st["link"][0] == -1 and st["back"][6] == 2
    for k in range(60):
        if rng.random() < 0.5:
            trio.feed(gen.step([int(e) for e in rng.permutation(5)[:int(rng.integers(1, 6))]]))
        else:
            trio.feed(gen.step([100 + int(e) for e in rng.permutation(3)[:int(rng.integers(1, 4))]]), via="extend")
            if trio.buf._n_staged > 4:                  # (a flush carries at most `capacity` rows: extend()'s own limit)
                trio.buf.flush()
        if k % 13 == 12:
            trio.bump(rng)
    st = trio.check()
    assert trio.buf._serial == trio.rows and (st["link"] >= 0).any()


def test_device_side_duplicate_ids_set_the_status_bit(dev):
    """A device id array cannot be checked without a sync: the kernel finds the repeat, sets the sticky bit, stores every row
    of the repeated stream unlinked and closes that stream; size, cursor and the other streams are untouched by it."""
    from prism_amd import _native as N
    from prism_amd.experience import HipReplayBuffer
    rng = np.random.default_rng(8)
    gen = Streams(rng, (7,))
    buf = HipReplayBuffer(32, 8, device=dev, n_step=3, use_per=True)

    def put(ids):
        r = gen.step(ids, force_open=True)
        return buf.extend_batch(r["obs"], r["next_obs"], r["action"], r["reward"], r["done"], r["trunc"],
                                stream_ids=torch.tensor(ids, device=dev))
    assert put([0, 1, 2, 3]) == 0
    buf.check_status()
    assert put([0, 1, 1, 2]) == 4                       # stream 1 twice
    torch.cuda.synchronize()
    assert int(buf.status.item()) & N.STATUS_INGEST_DUP_STREAM
    with pytest.raises(RuntimeError, match="stream_ids"):
        buf.check_status()
    assert len(buf) == 8 and buf.buffer._writer._cursor == 8 and buf._serial == 8
    back, link = buf.back.cpu().numpy(), buf.link.cpu().numpy()
    assert list(back[4:8]) == [0, -1, -1, 2] and link[1] == -1 and link[0] == 4 and link[2] == 7
    assert put([1, 0, 2]) == 8                          # stream 1 was closed: unlinked; the others go on
    assert put([3, 70]) == 11                           # id 70 lies outside the 64-entry table: stored unlinked
    assert put([70, 3]) == 13
    torch.cuda.synchronize()
    back = buf.back.cpu().numpy()
    assert list(back[8:15]) == [-1, 4, 7, 3, -1, -1, 11] and len(buf) == 15
    t = buf.tree.cpu().numpy()
    cap2 = buf.tree_capacity
    assert (t[cap2:cap2 + 15] == 1.0).all() and t[1, 0] == 15.0 and t[1, 1] == 1.0
    assert (buf.flags[:15].cpu().numpy() == 4).all()


def test_sample_and_gather_equal_the_twins(dev):
    """After a fill through extend_batch: gather() of every slot (n-step returns walk the links made on the device) and
    sample() (same seed, same draw count) give the twin's batches, and the oracle's n-step values."""
    rng = np.random.default_rng(6)
    trio, st = _lockstep(dev, 64, 3, 40, seed=6)
    idx = np.arange(64)
    got = {k: v.clone() for k, v in _flat(trio.buf.gather(idx)).items()}
    want = _flat(trio.twin.gather(idx))
    torch.cuda.synchronize()
    for k in want:
        assert torch.equal(got[k], want[k]), k
    out = trio.orc.gather(idx)
    np.testing.assert_array_equal(got["next/reward"].cpu().numpy().ravel(), out["reward"])
    np.testing.assert_array_equal(got["gamma"].cpu().numpy().ravel(), out["gamma"])
    np.testing.assert_array_equal(got["next/observation"].cpu().numpy().reshape(64, -1), out["next_obs"])
    assert len(np.unique(out["gamma"])) > 1                             # walks of different lengths were taken
    (b0, i0), (b1, i1) = trio.buf.sample(return_info=True), trio.twin.sample(return_info=True)
    torch.cuda.synchronize()
    assert torch.equal(i0["index"], i1["index"]) and torch.equal(i0["_weight"], i1["_weight"])
    for (k, a), (_, b) in zip(_flat(b0).items(), _flat(b1).items()):
        assert torch.equal(a, b), k


def _flat(batch, pre=""):
    out = {}
    for k, v in batch.items():
        if isinstance(v, dict):
            out.update(_flat(v, pre + k + "/"))
        else:
            out[pre + k] = v
    return out


def test_save_load_round_trip_and_empty(dev, tmp_path):
    from prism_amd.experience import HipReplayBuffer
    rng = np.random.default_rng(12)
    trio, st = _lockstep(dev, 100, 2, 13, seed=12)
    trio.bump(rng)
    st = trio.check()
    buf = trio.buf
    buf.save(str(tmp_path))
    new = HipReplayBuffer(100, 8, device=dev, n_step=3, gamma=0.99, use_per=True, seed=11)
    new.load(str(tmp_path))
    torch.cuda.synchronize()
    assert len(new) == len(buf) == 26 and new.buffer._writer._cursor == buf.buffer._writer._cursor == 26
    assert new._serial == 26 and new._stream_tab is None
    for name in ("obs", "succ_obs", "reward", "action", "link", "back", "per_state", "tree"):
        assert torch.equal(getattr(buf, name).cpu(), getattr(new, name).cpu()), name
    # an open chain's last row is written truncated, as the reference's save does; everything else unchanged
    f0, f1 = st["flags"][:26], new.flags[:26].cpu().numpy()
    open_end = ((f0 & 4) != 0) & ((f0 & 2) == 0) & (st["link"][:26] < 0)
    np.testing.assert_array_equal(f1, f0 | (2 * open_end).astype(np.uint8))
    # empty(): the next fill starts clean (table cleared, serial and cursor at 0) -- for the twin and the oracle alike
    gen = Streams(rng, (10, 10, 4))
    trio.feed(gen.step(range(2), force_open=True))                      # leave open rows behind
    trio.buf.empty()
    trio.twin.empty()
    trio.reset_tracking()
    assert buf._serial == 0 and len(buf) == 0 and int((buf._stream_tab >= 0).sum()) == 0
    for _ in range(15):                              # (30 rows: past the 28 stale rows, which the fresh oracle never saw)
        trio.feed(gen.step(range(2)))
    st = trio.check()
    assert (st["back"][:2] == -1).all()


def test_fill_replay_then_extend_batch(dev):
    """The library's own bulk loader rewrites the ring behind the stream table: after it the serial follows the cursor, no
    stream has an open row, and extend_batch goes on from there -- equal to a twin filled the same way and fed by extend()."""
    from prism_amd.synthetic import fill_replay
    rng = np.random.default_rng(14)
    trio, gen = Trio(dev, 64, (10, 10, 4), oracle=False), Streams(rng, (10, 10, 4))
    trio.feed(gen.step(range(3), force_open=True))                     # open rows the fill must forget
    for b in (trio.buf, trio.twin):
        fill_replay(b, 40, seed=3)
    trio.cur, trio.rows = {}, 40
    assert trio.buf._serial == 40 and int((trio.buf._stream_tab >= 0).sum()) == 0
    s = trio.feed(gen.step(range(3), force_open=True))
    st = trio.check()
    assert s == 40 and (st["back"][40:43] == -1).all()
    for _ in range(20):                                                # wraps over the filled rows
        trio.feed(gen.step(range(3)))
    trio.check()


def test_device_side_ids_after_reserve_streams(dev):
    """Device-side ids cannot grow the table (no sync): reserve_streams() sizes it, and ids up to that size then link."""
    rng = np.random.default_rng(15)
    trio, gen = Trio(dev, 23, (7,)), Streams(rng, (7,))
    trio.buf.reserve_streams(1000)
    assert trio.buf._stream_tab.numel() == 1024
    for _ in range(12):
        trio.feed(gen.step([999, 3, 64, 500]), place="device")
    st = trio.check()
    assert (st["link"] >= 0).any()


class VectorStubCollector:
    """A vectorised collector's surface: N environments in lockstep, ONE Agent.forward and ONE extend_batch per step.
    Observations go in as bool arrays, actions as the device tensor Agent.forward returned, the rest as NumPy arrays."""

    def __init__(self, n_env=8, C=4, n_actions=6, seed=0, p_done=0.05):
        self.n_env, self.C, self.A, self.p_done = n_env, C, n_actions, p_done
        self.rng = np.random.default_rng(seed)
        self.obs = None
        self.started = self.closed = False
        self.n_forward = self.n_batches = 0

    def _obs(self, n):
        return self.rng.random((n, 10, 10, self.C)) < 0.1

    def get_env_info(self):
        return (10, 10, self.C), self.A, 1

    def signal_processes_start_collecting(self, agent):
        self.started = True

    def collect_timesteps(self, n_timesteps, agent, exp_buffer, random=False):
        if self.obs is None:
            self.obs = self._obs(self.n_env)
        got = 0
        while got < n_timesteps:
            if random:
                acts = self.rng.integers(0, self.A, self.n_env)
            else:
                acts = agent.forward(self.obs.astype(np.float32))
                self.n_forward += 1
            nxt = self._obs(self.n_env)
            done = self.rng.random(self.n_env) < self.p_done
            trunc = ~done & (self.rng.random(self.n_env) < 0.02)
            exp_buffer.extend_batch(self.obs, nxt, acts, self.rng.standard_normal(self.n_env).astype(np.float32), done, trunc)
            self.n_batches += 1
            self.obs = np.where((done | trunc)[:, None, None, None], self._obs(self.n_env), nxt)
            got += self.n_env
        return got

    def log(self, logger):
        logger.log_data(data=0.0, group_name="Report/Rewards", var_name="Training Reward")

    def close(self):
        self.closed = True


@pytest.mark.parametrize("base", [2, 0])
def test_learn_with_a_vector_collector(dev, tmp_path, base):
    """Learner.learn() end to end, fed only through extend_batch: base 2 = IQN + PER (n-step 3), base 0 = DQN on uniform
    replay.  The loop acts, ingests, runs fused steps; the ring holds what was collected, with links, and no status bit."""
    from prism_amd.config import baseline_config
    from prism_amd.learner import Learner
    n_iter = 60
    cfg = baseline_config(base, device=dev, batch_size=32, experience_replay_capacity=2048, num_initial_random_timesteps=256,
                          timesteps_per_iteration=8, timestep_limit=256 + 8 * n_iter, timesteps_per_report=400,
                          timesteps_between_evaluations=300, target_update_period=40, checkpoint_dir=str(tmp_path),
                          log_to_wandb=False)
    col, ln = VectorStubCollector(seed=5), Learner()
    with contextlib.redirect_stdout(io.StringIO()):
        ln.configure(cfg, collector=col)
        agent, buf = ln.agent, ln.experience_buffer
        p0 = agent.flat.clone()
        real_empty = buf.empty
        buf.empty = lambda: None                 # learn() empties the buffer on exit: keep it for the checks below
        ln.learn()
        buf.empty = real_empty
    torch.cuda.synchronize()
    total = 256 + 8 * n_iter
    assert col.started and col.closed and col.n_forward == n_iter and col.n_batches == total // 8
    assert ln.cumulative_timesteps == total and ln.cumulative_model_updates == n_iter
    assert len(buf) == total and buf._serial == total and buf.buffer._writer._cursor == total
    assert torch.isfinite(agent.flat).all() and not torch.equal(agent.flat, p0)
    assert int(buf.status.item()) == 0
    buf.check_status()
    agent.check_status()
    link, back, flags = buf.link[:total].cpu().numpy(), buf.back[:total].cpu().numpy(), buf.flags[:total].cpu().numpy()
    ended = (flags & 3) != 0
    # lockstep, no wrap: every row but the last step's links 8 slots ahead exactly when its episode goes on
    want = np.where(~ended[:total - 8], np.arange(8, total), -1)
    np.testing.assert_array_equal(link[:total - 8], want)
    np.testing.assert_array_equal(back[8:], np.where(~ended[:total - 8], np.arange(total - 8), -1))
    assert ended.sum() > 10 and ((flags & 4) != 0)[~((flags & 1) != 0) | ((flags & 2) != 0)].all()
    if cfg.use_per:
        leaves = buf.sum_tree[buf.tree_capacity:buf.tree_capacity + total].cpu().numpy()
        assert (leaves > 0).all() and len(np.unique(leaves)) > 10
