"""GPU: reward clipping and episode returns inside ``extend_batch``'s launch -- ``prism_replay_ingest_tracked``,
``HipReplayBuffer.track_episodes`` / ``episode_stats``, ``prism_amd.collectors.VectorCollector``.

Two bars.  The ring: a tracked, clamping buffer fed RAW rewards equals, bit for bit in integer views (rows, flags, links,
trees whole, per_state, stream table, status), an untracked buffer fed host-clamped rewards through the unchanged
``prism_replay_ingest`` -- which ``tests/test_gpu_ingest.py``'s ``Trio`` in turn holds to an ``extend()``-fed twin and to the
row-by-row oracle.  The bookkeeping: ``episode_stats()`` and the per-stream accumulators equal ``EpisodeHost``
(tests/episode_cases.py, itself held to the live reference's recorded numbers) in exact float64 / integer equality."""
import contextlib
import io

import numpy as np
import pytest
import torch

from tests import episode_cases as EC
from tests.test_gpu_ingest import FIELDS, Streams, Trio

pytestmark = pytest.mark.gpu

EMA = 0.9


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return "cuda:0"


def _buffer(dev, capacity, use_per=True, clip="dopamine_clamp", track=True, **kw):
    from prism_amd.experience import HipReplayBuffer
    b = HipReplayBuffer(capacity, 8, device=dev, n_step=3, gamma=0.99, use_per=use_per, seed=11, reward_clipping_type=clip)
    if track:
        b.track_episodes(EMA, **kw)
    return b


_ON_DEVICE = {"host": (), "device": ("obs", "next_obs", "action", "reward", "done", "truncated", "ids"),
              "mixed": ("obs", "next_obs", "action", "done")}


def _put(buf, r, place="host", obs_mode="f32", pass_ids=True):
    """One extend_batch call of the transitions `r` (a Streams.step record), arguments on the host, on the device (action
    int64, flags torch.bool, as an agent and a device environment hand them over) or some of each."""
    cast = {"f32": np.float32, "u8": np.uint8, "bool": np.bool_}[obs_mode]
    a = dict(obs=r["obs"].astype(cast), next_obs=r["next_obs"].astype(cast), action=r["action"], reward=r["reward"],
             done=r["done"], truncated=r["trunc"])
    ids = np.asarray(r["ids"], np.int64) if pass_ids else None
    for k in _ON_DEVICE[place]:
        if k == "ids":
            ids = None if ids is None else torch.from_numpy(ids).to(buf.device)
        else:
            a[k] = torch.from_numpy(a[k]).to(buf.device)
            if k == "action":
                a[k] = a[k].long()
    return buf.extend_batch(stream_ids=ids, **a)


def _ints(t):
    x = t.cpu().numpy()
    return x.view({4: np.int32, 8: np.int64}[x.itemsize]) if x.dtype.kind == "f" else x


def assert_same_ring(got, want):
    """Everything extend_batch writes, in integer views (NaN rewards and -0.0 compare by bit pattern)."""
    for b in (got, want):
        b.flush()
    torch.cuda.synchronize()
    for k in FIELDS + ("status", "_stream_tab"):
        a, b = getattr(got, k), getattr(want, k)
        assert (a is None) == (b is None), k
        if a is not None:
            np.testing.assert_array_equal(_ints(a), _ints(b), err_msg=k)
    assert (len(got), got._serial, got.buffer._writer._cursor) == (len(want), want._serial, want.buffer._writer._cursor)


def _same_f64(got, want):
    """Bit equality -- except that a NaN the arithmetic MADE (inf - inf) carries the sign bit of the machine that made it,
    so two NaNs count as equal.  (The NaN rewards the ring stores are copies, and are compared by bit pattern.)"""
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    return bool(((EC.bits64(got) == EC.bits64(want)) | (np.isnan(got) & np.isnan(want))).all())


def assert_episodes(buf, host):
    """episode_stats() and the accumulators against the host restatement: exact."""
    torch.cuda.synchronize()
    got, want = buf.episode_stats(), host.stats()
    assert got.keys() == want.keys() == {"episodes", "training_reward", "mean_return", "mean_length", "last_return", "rows"}
    for k in want:
        if isinstance(want[k], float):
            assert got[k] is not None and _same_f64(got[k], want[k]), (k, got[k], want[k])
        else:
            assert got[k] == want[k] and type(got[k]) is type(want[k]), (k, got[k], want[k])
    size = buf._stream_tab.numel()
    assert buf._ep_return.numel() == buf._ep_length.numel() == size
    ret, length = host.accumulators(size)
    assert _same_f64(buf._ep_return.cpu().numpy(), ret), (buf._ep_return.cpu().numpy(), ret)
    np.testing.assert_array_equal(buf._ep_length.cpu().numpy(), length)
    return got


class Rig:
    """The tracked, clamping buffer under test beside a ``Trio`` whose extend_batch buffer is the UNTRACKED twin: the Trio is
    fed the host-clamped rewards (and checks itself against its extend() twin and the oracle), the buffer the raw ones."""

    def __init__(self, dev, capacity, obs_shape, use_per=True, oracle=True, reward_scale=3.0):
        self.trio = Trio(dev, capacity, obs_shape, use_per=use_per, oracle=oracle)
        self.buf = _buffer(dev, capacity, use_per)
        self.host = EC.EpisodeHost(EMA, clip="dopamine_clamp")
        self.scale = np.float32(reward_scale)
        assert self.trio.buf._ep is None and self.trio.buf._clip == 0

    def feed(self, r, place="host", obs_mode="f32", pass_ids=True):
        r = dict(r, reward=(r["reward"] * self.scale).astype(np.float32))      # a third of them beyond +-1
        first = self.trio.feed(dict(r, reward=EC.clamp_f32(r["reward"])), place="host" if place == "mixed" else place,
                               obs_mode=obs_mode, pass_ids=pass_ids)
        assert _put(self.buf, r, place, obs_mode, pass_ids) == first
        self.host.step_batch(r["ids"], r["reward"], r["done"], r["trunc"])

    def bump(self, rng, B=8):
        """A priority writeback on all of them, so that the default priority moves."""
        if not self.trio.use_per:
            return
        self.buf.flush()
        idx, td = rng.integers(0, len(self.buf), B), (rng.random(B) * 4).astype(np.float32)
        for b in (self.buf, self.trio.buf, self.trio.twin):
            b.update_priority(torch.from_numpy(idx).to(b.device), torch.from_numpy(td).to(b.device))
        if self.trio.orc is not None:
            self.trio.orc.sampler.update_priority(idx, td)

    def check(self):
        st = self.trio.check()
        assert_same_ring(self.buf, self.trio.buf)
        return st, assert_episodes(self.buf, self.host)


def _lockstep(dev, capacity, n, steps, seed, obs_shape=(7,), use_per=True, oracle=True, p_done=0.07, p_trunc=0.03, **feed_kw):
    rng = np.random.default_rng(seed)
    rig, gen = Rig(dev, capacity, obs_shape, use_per=use_per, oracle=oracle), Streams(rng, obs_shape, p_done, p_trunc)
    for k in range(steps):
        rig.feed(gen.step(range(n)), **feed_kw)
        if k % 17 == 16:
            rig.bump(rng)
    return (rig,) + rig.check()


def test_one_stream_forty_steps(dev):
    rig, st, ep = _lockstep(dev, 64, 1, 40, seed=1, pass_ids=False, p_done=0.2, p_trunc=0.1)
    assert ep["rows"] == 40 and ep["episodes"] >= 2 and np.abs(st["reward"][:40]).max() == 1.0


@pytest.mark.parametrize("use_per", [True, False])
def test_five_streams_subsets_absences_and_table_growth(dev, use_per):
    """Non-identity ids, a subset of random size per call, a ring of 23 rows that a stream's absence outlasts, and ids that
    make the stream table -- and the accumulators with it, open episodes kept -- grow from 64 to 4096 entries."""
    rng = np.random.default_rng(23)
    rig, gen = Rig(dev, 23, (10, 10, 4), use_per=use_per), Streams(rng, (10, 10, 4), p_done=0.05, p_trunc=0.02)
    labels = [5, 0, 63, 999, 4000]
    for k in range(150):
        pool = labels[:3] if k < 20 else labels
        if 60 <= k < 100:
            pool = [e for e in pool if e != 5]               # stream 5 stays away for 40 calls (its ring rows are long gone)
        ids = [int(e) for e in rng.permutation(pool)[:int(rng.integers(1, len(pool) + 1))]]
        if k == 20:
            ids = [999, 63]                                  # the first id beyond the 64-entry table
        if k == 59:
            ids = [5, 0]
        rig.feed(gen.step(ids, force_open=k == 59))
        if k == 19:
            assert rig.buf._stream_tab.numel() == rig.buf._ep_return.numel() == 64
            open_before = rig.buf._ep_length.cpu().numpy().copy()
        if k == 20:
            assert rig.buf._stream_tab.numel() == rig.buf._ep_return.numel() == 1024
            torch.cuda.synchronize()
            kept = rig.buf._ep_length[:64].cpu().numpy()
            assert ((kept == open_before) | np.isin(np.arange(64), ids)).all()
        if k == 59:
            away = int(rig.buf._ep_length[5].item())
            assert away >= 1
        if k == 99:
            assert int(rig.buf._ep_length[5].item()) == away     # an absent stream's open episode waits for it
        if k % 29 == 28:
            rig.bump(rng)
    st, ep = rig.check()
    assert rig.buf._stream_tab.numel() == 4096 and ep["episodes"] > 10 and (st["link"] >= 0).any()


def test_pass_boundaries_of_1024_rows_and_n_equal_capacity(dev):
    """Calls of 2048 (= capacity), 1025 and 2048 rows: the episode role walks them in passes of 1024 rows.  Episode ends are
    forced into rows 1023 and 1024 (both sides of the boundary), the last row of every call, and sprinkled elsewhere, so
    the order in which the EMA takes them up crosses passes."""
    rng = np.random.default_rng(31)
    rig, gen = Rig(dev, 2048, (7,)), Streams(rng, (7,), p_done=0.1, p_trunc=0.05)
    for n in (2048, 1025, 2048, 1025):
        r = gen.step(range(n))
        for i in (0, 1023, 1024, n - 1):
            r["done"][i] = True
            gen.carry.pop(i, None)
        r["trunc"][1023] = True
        rig.feed(r, pass_ids=False)
    st, ep = rig.check()
    assert ep["rows"] == 2 * 2048 + 2 * 1025 and ep["episodes"] > 500


@pytest.mark.parametrize("capacity,n,steps", [(300, 129, 6), (33, 33, 4)])
def test_a_launch_of_256_threads_and_a_whole_small_ring(dev, capacity, n, steps):
    """129 rows: the launch has 256 threads, the second wave pair holds one row.  33 = capacity: every call rewrites the ring."""
    rig, st, ep = _lockstep(dev, capacity, n, steps, seed=n, pass_ids=False)
    assert ep["rows"] == n * steps and ep["episodes"] > 5


@pytest.mark.parametrize("obs_shape,obs_mode,place", [((7,), "f32", "host"), ((7,), "u8", "device"), ((10, 10, 4), "bool", "mixed"),
                                                      ((10, 10, 4), "f32", "device"), ((10, 10, 4), "u8", "host"),
                                                      ((7,), "bool", "device"), ((7,), "f32", "mixed")])
def test_observation_kinds_and_argument_placement(dev, obs_shape, obs_mode, place):
    rig, st, ep = _lockstep(dev, 23, 3, 25, seed=3, obs_shape=obs_shape, obs_mode=obs_mode, place=place)
    assert ep["rows"] == 75


def test_reward_edge_values_by_bit_pattern(dev):
    """0, -0.0, +-1, the float32 neighbours of +-1 on both sides, +-inf and NaN (two payloads): what the ring stores equals the
    host clamp bit for bit -- NaN and -0.0 pass through -- and the returns, NaN and infinities included, equal the host's."""
    one = np.float32(1)
    nan2 = np.array([0x7fc00001], np.uint32).view(np.float32)[0]
    edge = np.array([0.0, -0.0, 1.0, -1.0, np.nextafter(one, np.float32(0)), np.nextafter(one, np.float32(2)),
                     np.nextafter(-one, np.float32(0)), np.nextafter(-one, np.float32(-2)), np.inf, -np.inf, np.nan, nan2,
                     2.5, -0.5], np.float32)
    n = len(edge)
    rng = np.random.default_rng(2)
    gen = Streams(rng, (7,))
    buf, twin, host = _buffer(dev, 64), _buffer(dev, 64, clip=None, track=False), EC.EpisodeHost(EMA, clip="dopamine_clamp")
    for k in range(4):
        r = gen.step(range(n), force_open=True)
        r["reward"] = np.roll(edge, k)                       # every stream meets several of them, NaN and inf in its sum
        if k == 3:
            r["done"][:] = True
        _put(buf, r, pass_ids=False)
        _put(twin, dict(r, reward=EC.clamp_f32(r["reward"])), pass_ids=False)
        host.step_batch(r["ids"], r["reward"], r["done"], r["trunc"])
    assert_same_ring(buf, twin)
    stored = buf.reward[:n].cpu().numpy()
    want = np.array([host.stored(x) for x in edge], np.float32)
    np.testing.assert_array_equal(EC.bits32(stored), EC.bits32(want))
    assert EC.bits32(stored[1]) == EC.bits32(np.float32(-0.0)) and EC.bits32(stored[11]) == 0x7fc00001
    assert list(stored[[5, 7, 8, 9]]) == [1.0, -1.0, 1.0, -1.0] and stored[4] < 1.0 and stored[6] > -1.0
    ep = assert_episodes(buf, host)
    assert ep["episodes"] == n and np.isnan(ep["training_reward"])


def test_device_side_ids_repeated_and_beyond_the_table(dev):
    """A device id array with a repeated id and one beyond the 64-entry table: the status bit is set, those rows are not
    tracked, the repeated stream's accumulators are zeroed (it is closed), the others go on -- and the ring is the twin's."""
    from prism_amd import _native as N
    rng = np.random.default_rng(8)
    gen = Streams(rng, (7,))
    buf, twin, host = _buffer(dev, 32), _buffer(dev, 32, clip=None, track=False), EC.EpisodeHost(EMA, clip="dopamine_clamp")

    def put(ids, untracked=(), ends=()):
        r = gen.step(ids, force_open=True)
        r["reward"] = (r["reward"] * 3).astype(np.float32)
        for i in ends:
            r["done"][i] = True
        _put(buf, r, place="device")
        _put(twin, dict(r, reward=EC.clamp_f32(r["reward"])), place="device")
        host.step_batch(ids, r["reward"], r["done"], r["trunc"], untracked=untracked)
    put([0, 1, 2, 3])
    put([0, 1, 2, 3])
    assert_episodes(buf, host)
    assert int(buf._ep_length[1].item()) == 2
    put([0, 1, 1, 2], untracked=(1, 2))                      # stream 1 twice
    host.close(1)
    assert int(buf.status.item()) & N.STATUS_INGEST_DUP_STREAM
    assert_episodes(buf, host)
    assert int(buf._ep_length[1].item()) == 0 and float(buf._ep_return[1].item()) == 0.0
    put([3, 70, 1], untracked=(1,), ends=(0,))               # id 70 lies beyond the table; stream 1 starts over; 3 ends
    put([70, 0], untracked=(0,), ends=(1,))
    assert_same_ring(buf, twin)
    ep = assert_episodes(buf, host)
    assert ep["rows"] == 4 + 4 + 2 + 2 + 1 and ep["episodes"] == 2
    with pytest.raises(RuntimeError, match="stream_ids"):
        buf.check_status()


def test_extend_rows_between_calls_are_neither_tracked_nor_clipped(dev):
    """Timestep chains through extend() between vector steps: stored as handed over (their collector has clipped already),
    not counted, and the vector streams' episodes go on across them."""
    rng = np.random.default_rng(4)
    rig, gen = Rig(dev, 37, (10, 10, 4)), Streams(rng, (10, 10, 4))
    chains = Streams(np.random.default_rng(5), (10, 10, 4))
    n_extend = 0
    for k in range(40):
        rig.feed(gen.step([int(e) for e in rng.permutation(5)[:int(rng.integers(1, 6))]]))
        if k % 3 == 0:
            r = chains.step([100 + int(e) for e in rng.permutation(3)[:2]])
            r["reward"] = (r["reward"] * 5).astype(np.float32)
            ts = rig.trio._timesteps(r)                       # the same Timestep objects to all three buffers
            _extend_all(rig, ts, r)
            n_extend += len(ts)
    st, ep = rig.check()
    assert np.abs(st["reward"]).max() > 1.0 and ep["rows"] == rig.trio.rows - n_extend and n_extend > 20


def _extend_all(rig, ts, r):
    """What Trio.feed(via="extend") does, for three buffers: the rows through extend(), and the oracle's bookkeeping."""
    t = rig.trio
    for b in (rig.buf, t.buf, t.twin):
        for x in ts:
            b.extend(x)
        b.flush()
    for i, e in enumerate(r["ids"]):
        slot = t.rows % t.cap
        t.owner[slot] = t.rows
        rec = t.pending.pop(e, None)
        prev = rec[0] if rec is not None and t.owner[rec[0]] == rec[1] else -1
        done, trunc = bool(r["done"][i]), bool(r["trunc"][i])
        has_next = trunc or not done
        if t.orc is not None:
            assert t.orc.insert(r["obs"][i], r["next_obs"][i] if has_next else None, r["reward"][i], r["action"][i], done, trunc,
                                has_next, prev) == slot
        if not done and not trunc:
            t.pending[e] = (slot, t.rows)
        t.rows += 1


# ---------------------------------------------------------------------------------------------------- resets
def _open_run(dev, buf, host, gen, steps, n=4):
    for _ in range(steps):
        r = gen.step(range(n))
        r["reward"] = (r["reward"] * 3).astype(np.float32)
        _put(buf, r, pass_ids=False)
        host.step_batch(r["ids"], r["reward"], r["done"], r["trunc"])


@pytest.mark.parametrize("how", ["empty", "load_arrays", "fill_replay"])
def test_resets_close_the_open_episodes_and_keep_the_statistics(dev, how):
    rng = np.random.default_rng(12)
    gen = Streams(rng, (10, 10, 4))
    buf, host = _buffer(dev, 64), EC.EpisodeHost(EMA, clip="dopamine_clamp")
    _open_run(dev, buf, host, gen, 30)
    before = assert_episodes(buf, host)
    assert before["episodes"] > 3 and int((buf._ep_length > 0).sum().item()) > 0      # cut in mid-episode
    if how == "empty":
        buf.empty()
    elif how == "load_arrays":
        z = torch.zeros(5, 400)
        buf.load_arrays(z, z, torch.zeros(5), torch.zeros(5, dtype=torch.int32), torch.full((5,), 4, dtype=torch.uint8),
                        torch.full((5,), -1, dtype=torch.int32), priorities=torch.ones(5))
    else:
        from prism_amd.synthetic import fill_replay
        fill_replay(buf, 20, seed=3)
    host.close()
    gen.carry.clear()
    assert int((buf._ep_length != 0).sum().item()) == 0 and float(buf._ep_return.abs().sum().item()) == 0.0
    assert assert_episodes(buf, host) == before
    _open_run(dev, buf, host, gen, 20)                       # and on it goes: first steps of new episodes, the EMA continued
    after = assert_episodes(buf, host)
    assert after["episodes"] > before["episodes"]


def test_track_episodes_twice(dev):
    buf = _buffer(dev, 16)
    buf.track_episodes(EMA)                                  # the same parameters: nothing happens
    for kw in (dict(ema=0.5), dict(ema=EMA, count_first_step=True)):
        with pytest.raises(ValueError, match="already tracking"):
            buf.track_episodes(**kw)


def test_count_first_step_on_the_device(dev):
    rng = np.random.default_rng(6)
    gen = Streams(rng, (7,))
    buf, host = _buffer(dev, 64, count_first_step=True), EC.EpisodeHost(EMA, count_first_step=True, clip="dopamine_clamp")
    _open_run(dev, buf, host, gen, 30)
    assert assert_episodes(buf, host)["episodes"] > 3


def test_clamp_without_tracking_and_tracking_without_clamp(dev):
    """Either of the two takes the tracked entry point; the ring is the twin's both times."""
    rng = np.random.default_rng(9)
    gen = Streams(rng, (7,))
    clamp_only, track_only = _buffer(dev, 32, track=False), _buffer(dev, 32, clip="dopamine_clip")
    twin_clamped, twin_raw = _buffer(dev, 32, clip=None, track=False), _buffer(dev, 32, clip=("dopamine clamp",), track=False)
    host = EC.EpisodeHost(EMA)
    for _ in range(20):
        r = gen.step(range(3))
        r["reward"] = (r["reward"] * 3).astype(np.float32)
        for b in (clamp_only, track_only, twin_raw):
            _put(b, r, pass_ids=False)
        _put(twin_clamped, dict(r, reward=EC.clamp_f32(r["reward"])), pass_ids=False)
        host.step_batch(r["ids"], r["reward"], r["done"], r["trunc"])
    assert_same_ring(clamp_only, twin_clamped)
    assert_same_ring(track_only, twin_raw)
    assert clamp_only._ep is None and float(track_only.reward.abs().max().item()) > 1.0
    assert_episodes(track_only, host)


# ---------------------------------------------------------------------------------------------------- exact resume
def test_resume_in_mid_episode_continues_bit_identically(dev, tmp_path):
    rng = np.random.default_rng(13)
    gen = Streams(rng, (10, 10, 4))
    buf, host = _buffer(dev, 64), EC.EpisodeHost(EMA, clip="dopamine_clamp")
    _open_run(dev, buf, host, gen, 25)
    assert int((buf._ep_length > 0).sum().item()) > 0
    snap = buf.save_state(tmp_path / "snap")
    from prism_amd.util import snapshot
    part = snapshot.read_snapshot(snap, ["replay"])[0]["replay"]
    assert sorted(part["episodes"]) == ["count_first_step", "counts", "ema", "ep_length", "ep_return", "stats"]
    new = _buffer(dev, 64, track=False)                      # fresh, tracking off: the snapshot turns it on
    new.load_state(snap)
    assert new._ep == dict(ema=EMA, count_first_step=False)
    assert_same_ring(new, buf)
    assert_episodes(new, host)
    for r in [gen.step(range(4)) for _ in range(25)]:
        r["reward"] = (r["reward"] * 3).astype(np.float32)
        for b in (buf, new):
            _put(b, r, pass_ids=False)
        host.step_batch(r["ids"], r["reward"], r["done"], r["trunc"])
    assert_same_ring(new, buf)
    assert assert_episodes(new, host) == assert_episodes(buf, host)


def test_keep_streams_false_zeroes_the_open_episodes(dev, tmp_path):
    rng = np.random.default_rng(14)
    gen = Streams(rng, (7,))
    buf, host = _buffer(dev, 64), EC.EpisodeHost(EMA, clip="dopamine_clamp")
    _open_run(dev, buf, host, gen, 25)
    before = assert_episodes(buf, host)
    snap = buf.save_state(tmp_path / "snap")
    closed = _buffer(dev, 64, track=False)
    closed.load_state(snap, keep_streams=False)
    host.close()
    gen.carry.clear()
    assert int((closed._ep_length != 0).sum().item()) == 0 and int((closed._stream_tab >= 0).sum().item()) == 0
    assert assert_episodes(closed, host) == before           # what finished episodes added up is kept
    _open_run(dev, closed, host, gen, 10)
    assert_episodes(closed, host)


def test_untracked_snapshot_has_todays_keys_and_leaves_tracking_alone(dev, tmp_path):
    rng = np.random.default_rng(15)
    gen = Streams(rng, (7,))
    plain = _buffer(dev, 64, clip=None, track=False)
    for _ in range(5):
        _put(plain, gen.step(range(3)), pass_ids=False)
    part = plain._state_part()
    assert sorted(part) == sorted(["rows", "size", "obs_shape", "cursor", "serial", "obs_dtype", "obs", "succ_obs", "reward",
                                   "action", "flags", "link", "back", "per_state", "slot_id", "pending", "stream_tab", "seed",
                                   "draws", "alpha", "beta", "eps", "leaves"])
    snap = plain.save_state(tmp_path / "snap")
    tracked, host = _buffer(dev, 64), EC.EpisodeHost(EMA, clip="dopamine_clamp")
    tracked.load_state(snap)                                 # no "episodes" key: tracking stays as the buffer has it
    assert tracked._ep == dict(ema=EMA, count_first_step=False)
    assert_same_ring(tracked, plain)
    gen.carry.clear()
    _open_run(dev, tracked, host, gen, 10, n=3)
    assert_episodes(tracked, host)


# ---------------------------------------------------------------------------------------------------- learn()
class ToyEnvs:
    """Eight deterministic environments: observations, rewards and episode ends are functions of the step count alone, so a
    run can be restated on the host and continued from (k, cur) -- the environment's own state."""
    n_actions, obs_shape = 6, (10, 10, 4)

    def __init__(self, n=8, quiet_steps=40):
        self.n, self.k, self.quiet, self.cur, self.log, self.closed = n, 0, quiet_steps, None, [], False

    def _obs(self, salt):
        return (np.random.default_rng([7, self.k, salt]).random((self.n,) + self.obs_shape) < 0.1).astype(np.float32)

    def reset(self):
        self.cur = self._obs(0)
        return self.cur

    def step(self, actions):
        assert len(actions) == self.n
        self.k += 1
        k, i = self.k, np.arange(self.n)
        nxt = self._obs(1)
        reward = (((k * 7 + i * 3) % 11 - 5) * 0.75).astype(np.float32)          # -3.75 .. 3.75: most beyond the clamp
        done = (k >= self.quiet) & ((k + 3 * i) % 17 == 0)
        trunc = (k >= self.quiet) & ((k + 5 * i) % 29 == 0)
        self.log.append((reward, done, trunc))
        self.cur = np.where((done | trunc)[:, None, None, None], self._obs(2), nxt)
        return nxt, reward, done, trunc

    def observe(self):
        return self.cur

    def close(self):
        self.closed = True


def _toy_learn(dev, ckpt_dir, limit, resume_from=None, raise_limit_to=None):
    """learn() over ToyEnvs with a VectorCollector: (learner, environments, [(rows collected, logged training reward,
    logged episode count)] per report)."""
    from prism_amd.collectors import VectorCollector
    from prism_amd.config import baseline_config
    from prism_amd.learner import Learner
    cfg = baseline_config(2, device=dev, batch_size=32, experience_replay_capacity=2048, num_initial_random_timesteps=256,
                          timesteps_per_iteration=8, timestep_limit=limit, timesteps_per_report=8,
                          timesteps_between_evaluations=10 ** 6, target_update_period=40, checkpoint_dir=str(ckpt_dir),
                          log_to_wandb=False, reward_clipping_type="dopamine_clamp", backup_checkpoints=True)
    envs = ToyEnvs()
    col, ln, reports = VectorCollector(envs, cfg), Learner(), []
    with contextlib.redirect_stdout(io.StringIO()):
        ln.configure(cfg, collector=col)
        real = ln.logger.log_data
        seen = {}

        def log_data(data, group_name, var_name, *a, **kw):
            if group_name == "Report/Rewards":
                seen[var_name] = data
                if var_name == "Episodes":
                    reports.append((ln.cumulative_timesteps, seen["Training Reward"], data))
            return real(data, group_name, var_name, *a, **kw)
        ln.logger.log_data = log_data
        if resume_from is not None:
            envs.k, envs.cur = resume_from.k, resume_from.cur.copy()         # the environments' own business
            ln.load_state(ln.checkpointer.latest_backup())
            ln.timestep_limit = raise_limit_to
        ln.learn()
    torch.cuda.synchronize()
    return ln, envs, reports


@pytest.fixture(scope="module")
def toy_run(dev, tmp_path_factory):
    return _toy_learn(dev, tmp_path_factory.mktemp("toy_ref"), 256 + 8 * 60)


def _expected_reports(envs_log, rows_list, n=8):
    host, out, fed = EC.EpisodeHost(EMA, clip="dopamine_clamp"), [], 0
    for rows in rows_list:
        while fed < rows // n:
            reward, done, trunc = envs_log[fed]
            host.step_batch(range(n), reward, done, trunc)
            fed += 1
        out.append((rows, host.stats()["training_reward"], host.stats()["episodes"]))
    return out


def test_learn_logs_the_training_reward_of_the_host_restatement(dev, toy_run):
    ln, envs, reports = toy_run
    assert ln.cumulative_timesteps == 256 + 8 * 60 and envs.closed and len(envs.log) == 32 + 60
    assert [r[0] for r in reports] == [256 + 8 * (j + 1) for j in range(60)]
    want = _expected_reports(envs.log, [r[0] for r in reports])
    assert reports == want                                   # exact: float64 equality, None before the first episode end
    assert reports[0][1] is None and reports[0][2] == 0 and reports[-1][2] > 20 and isinstance(reports[-1][1], float)
    buf = ln.experience_buffer                               # (emptied on the way out: the statistics are kept)
    assert buf.episode_stats()["rows"] == 256 + 8 * 60 and buf._clip == 1


def test_learn_resumed_from_a_snapshot_reports_the_same(dev, toy_run, tmp_path):
    _, _, want = toy_run
    first, envs1, rep1 = _toy_learn(dev, tmp_path, 256 + 8 * 25)
    assert first.checkpointer.latest_backup() is not None
    second, envs2, rep2 = _toy_learn(dev, tmp_path, 256 + 8 * 25, resume_from=envs1, raise_limit_to=256 + 8 * 60)
    assert second.agent is not first.agent and second.cumulative_timesteps == 256 + 8 * 60
    assert rep1 + rep2 == want
    assert second.timestep_collector.rows == 256 + 8 * 60
