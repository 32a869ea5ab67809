"""GPU: the byte observation ring -- ``HipReplayBuffer(obs_storage="uint8")``, the ``prism_*_ring`` entry points and their
kernels -- held to an fp32 TWIN fed the same stream, bit for bit (float tensors are compared through their int32 views).
The fp32 ring itself is held to the oracle and the reference's recordings by the other suites; cases and the host's
expectations come from tests/obs_ring_cases.py (shown on the CPU by tests/test_obs_ring_host.py)."""
import contextlib
import io
import itertools
import os
import weakref

import numpy as np
import pytest
import torch

from tests import obs_ring_cases as OC

pytestmark = pytest.mark.gpu

CAP, N_STREAMS, B = 37, 8, 16


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return "cuda:0"


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def _same(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.dtype, b.dtype, a.shape, b.shape)
    assert torch.equal(_bits(a), _bits(b)), what


def _buffer(dev, storage, capacity=CAP, batch=B, **kw):
    from prism_amd.experience import HipReplayBuffer
    return HipReplayBuffer(capacity, batch, device=dev, obs_storage=storage, **kw)


def _put(buf, st, conv=lambda x: x):
    return buf.extend_batch(conv(st["obs"]), conv(st["next_obs"]), st["action"], st["reward"], st["done"], st["truncated"])


def _batch_tensors(buf):
    return dict(obs=buf._obs, next_obs=buf._next_obs, reward=buf._reward, nonterminal=buf._nonterminal, gamma=buf._gamma,
                action=buf._action)


def _small_arrays(buf):
    out = {k: getattr(buf, k) for k in ("reward", "action", "flags", "link", "back", "per_state", "status")}
    if buf.use_per:
        out["tree"] = buf.tree
    return out


def _assert_same_ring(a, b, what):
    """Everything the two rings hold, the observation arrays widened where one of them is a byte ring."""
    for name in ("obs", "succ_obs"):
        _same(getattr(a, name).float(), getattr(b, name).float(), f"{what}: {name}")
    for k, v in _small_arrays(a).items():
        _same(v, _small_arrays(b)[k], f"{what}: {k}")
    assert (a._size, a._serial, a.buffer._writer._cursor) == (b._size, b._serial, b.buffer._writer._cursor), what
    np.testing.assert_array_equal(a._slot_id, b._slot_id)


def _assert_twin(u8, f32, what):
    """gather(every stored slot), one sample() batch with index and weights, both trees, the small arrays."""
    slots = np.arange(len(u8))
    u8.gather(slots), f32.gather(slots)
    for k, v in _batch_tensors(u8).items():
        _same(v, _batch_tensors(f32)[k], f"{what}: gather {k}")
    (_, iu), (_, if_) = u8.sample(return_info=True), f32.sample(return_info=True)
    _same(iu["index"], if_["index"], f"{what}: sampled index")
    if u8.use_per:
        _same(iu["_weight"], if_["_weight"], f"{what}: IS weights")
    for k, v in _batch_tensors(u8).items():
        _same(v, _batch_tensors(f32)[k], f"{what}: sample {k}")
    _assert_same_ring(u8, f32, what)


# ---------------------------------------------------------------------------------------------- 5. ring twin
@pytest.mark.parametrize("use_per", [True, False])
@pytest.mark.parametrize("n_step", [1, 3])
@pytest.mark.parametrize("shape", OC.SHAPES)
def test_byte_ring_equals_its_fp32_twin(dev, shape, n_step, use_per):
    u8, f32 = (_buffer(dev, s, n_step=n_step, use_per=use_per) for s in ("uint8", "float32"))
    gen = OC.Streams(shape, N_STREAMS, seed=11 + n_step)
    steps, fed, checks = [], 0, 0
    while fed < 3 * CAP:
        st = gen.step()
        steps.append(st)
        assert _put(u8, st) == _put(f32, st) == fed % CAP
        if (fed + N_STREAMS) // (CAP // 2) > fed // (CAP // 2):          # every half capacity
            _assert_twin(u8, f32, f"after {fed + N_STREAMS} rows")
            checks += 1
        fed += N_STREAMS
    assert checks >= 6 and len(u8) == CAP
    torch.cuda.synchronize()
    obs, succ, cursor = OC.expected_ring(CAP, steps)
    np.testing.assert_array_equal(u8.obs.cpu().numpy(), obs)
    np.testing.assert_array_equal(u8.succ_obs.cpu().numpy(), succ)
    assert u8.buffer._writer._cursor == cursor
    assert int(u8.status.item()) == 0 and int(f32.status.item()) == 0
    u8.check_status()


# ---------------------------------------------------------------------------------------------- 12. size
def test_byte_ring_is_a_quarter_of_the_bytes(dev):
    u8, f32 = _buffer(dev, "uint8"), _buffer(dev, "float32")
    st = OC.Streams((10, 10, 4), N_STREAMS, seed=1).step()
    _put(u8, st), _put(f32, st)
    for t in (u8.obs, u8.succ_obs):
        assert t.dtype is torch.uint8 and t.nbytes == CAP * 400 and t.shape == (CAP, 400)
    assert f32.obs.dtype is torch.float32 and f32.obs.nbytes == 4 * u8.obs.nbytes
    assert u8._desc.obs == u8.obs.data_ptr() and u8._desc.succ_obs == u8.succ_obs.data_ptr()
    assert u8._obs.dtype is torch.float32                           # the static batch stays fp32


# ---------------------------------------------------------------------------------------------- 6. input paths
def _extend_rows(buf, steps):
    """The same transitions as linked Timestep chains through extend(): weak reference to a live successor, a strong one to
    a truncation node, none behind an episode end."""
    from prism_amd.experience import Timestep
    ids, nodes, keep = itertools.count(), {}, []
    for st in steps:
        for i in range(st["obs"].shape[0]):
            t = nodes.pop(i, None) or Timestep(id=next(ids), obs=st["obs"][i].astype(np.float32))
            t.action, t.reward = int(st["action"][i]), float(st["reward"][i])
            t.done, t.truncated = bool(st["done"][i]), bool(st["truncated"][i])
            nxt = Timestep(id=next(ids), obs=st["next_obs"][i].astype(np.float32))
            if t.truncated:
                t.next = nxt
            elif not t.done:
                t.next, nxt.prev, nodes[i] = weakref.ref(nxt), weakref.ref(t), nxt
            buf.extend(t)
            keep.append(t)
        buf.flush()                                                   # (one insert batch holds at most `capacity` rows)


@pytest.mark.parametrize("values", ["bytes", "bool"])
@pytest.mark.parametrize("shape", [(10, 10, 4), (6,)])
def test_every_input_path_leaves_the_same_bytes(dev, shape, values):
    gen = OC.Streams(shape, N_STREAMS, seed=5)
    steps = [gen.step() for _ in range(6)]                            # 48 rows: the ring wraps
    if values == "bool":
        for st in steps:                                              # (thresholded: 0 / 1 planes, chains kept)
            st["obs"], st["next_obs"] = (st["obs"] > 100).astype(np.uint8), (st["next_obs"] > 100).astype(np.uint8)
    obs, succ, _ = OC.expected_ring(CAP, steps)
    on_dev = lambda f: (lambda x: torch.from_numpy(np.ascontiguousarray(f(x))).to(dev))
    paths = {"host uint8": lambda x: x, "host float32": lambda x: x.astype(np.float32),
             "device uint8": on_dev(lambda x: x), "device float32": on_dev(lambda x: x.astype(np.float32))}
    if values == "bool":
        paths.update({"host bool": lambda x: x.astype(bool), "device bool": on_dev(lambda x: x.astype(bool))})
    rings = {}
    for name, conv in paths.items():
        buf = _buffer(dev, "uint8")
        for st in steps:
            _put(buf, st, conv)
        rings[name] = buf
    rings["extend()"] = _buffer(dev, "uint8")
    _extend_rows(rings["extend()"], steps)
    torch.cuda.synchronize()
    for name, buf in rings.items():
        np.testing.assert_array_equal(buf.obs.cpu().numpy(), obs, err_msg=name)
        np.testing.assert_array_equal(buf.succ_obs.cpu().numpy(), succ, err_msg=name)
        _same(buf.flags, rings["host uint8"].flags, name)
        _same(buf.link, rings["host uint8"].link, name)
        assert int(buf.status.item()) == 0, name


# ---------------------------------------------------------------------------------------------- 7. inexact data
def _ring_image(buf):
    torch.cuda.synchronize()
    img = {k: v.clone() for k, v in _small_arrays(buf).items()}
    img.update(obs=buf.obs.clone(), succ_obs=buf.succ_obs.clone())
    return img, (buf._size, buf._serial, buf.buffer._writer._cursor, buf._n_staged, buf._slot_id.copy())


def _assert_untouched(buf, image):
    img, host = image
    now, host_now = _ring_image(buf)
    for k in img:
        _same(now[k], img[k], k)
    assert host[:4] == host_now[:4] and np.array_equal(host[4], host_now[4])


def _spoiled(x, row, col, bad):
    f = x.astype(np.float32)
    f.reshape(f.shape[0], -1)[row, col] = bad
    return f


@pytest.mark.parametrize("bad", OC.INEXACT)
@pytest.mark.parametrize("shape", [(10, 10, 4), (6,)])
def test_inexact_observations(dev, shape, bad):
    from prism_amd import _native as N
    from prism_amd.experience import Timestep
    buf = _buffer(dev, "uint8")
    gen = OC.Streams(shape, N_STREAMS, seed=9)
    first, st = gen.step(), gen.step()
    _put(buf, first)
    st["done"][5], st["truncated"][5] = False, False                  # (row 5 keeps its successor row)
    f_obs, f_next = _spoiled(st["obs"], 3, 4, bad), _spoiled(st["next_obs"], 5, 2, bad)
    # ---- from the host: a ValueError, and the ring is bit for bit what it was
    image = _ring_image(buf)
    for o, n in ((f_obs, st["next_obs"].astype(np.float32)), (st["obs"].astype(np.float32), f_next),
                 (f_obs, torch.from_numpy(st["next_obs"].astype(np.float32)).to(dev))):
        with pytest.raises(ValueError, match="byte-exact"):
            buf.extend_batch(o, n, st["action"], st["reward"], st["done"], st["truncated"])
    t = Timestep(id=10 ** 6, obs=f_obs[3], action=0, reward=0.0, done=True, truncated=False)
    with pytest.raises(ValueError, match="byte-exact"):
        buf.extend(t)
    with pytest.raises(ValueError, match="byte-exact"):
        buf.load_arrays(f_obs, st["next_obs"], st["reward"], st["action"], np.zeros(N_STREAMS, np.uint8),
                        np.full(N_STREAMS, -1, np.int32))
    _assert_untouched(buf, image)
    assert int(buf.status.item()) == 0
    # ---- in a device float tensor: stored as 0, the sticky bit, every other element intact
    to_dev = lambda x: torch.from_numpy(x).to(dev)
    buf.extend_batch(to_dev(f_obs), to_dev(f_next), st["action"], st["reward"], st["done"], st["truncated"])
    torch.cuda.synchronize()
    assert int(buf.status.item()) == N.STATUS_OBS_INEXACT
    with pytest.raises(RuntimeError, match="byte-exact"):
        buf.check_status()
    want = dict(st)
    want["obs"], want["next_obs"] = st["obs"].copy(), st["next_obs"].copy()
    want["obs"].reshape(N_STREAMS, -1)[3, 4] = 0
    want["next_obs"].reshape(N_STREAMS, -1)[5, 2] = 0
    obs, succ, _ = OC.expected_ring(CAP, [first, want])
    np.testing.assert_array_equal(buf.obs.cpu().numpy(), obs)
    np.testing.assert_array_equal(buf.succ_obs.cpu().numpy(), succ)


def test_insert_ring_narrows_float_staging(dev):
    """prism_replay_insert_ring with fp32 staging rows into a byte ring (the host layer stages bytes; another binding may
    not): narrowed, and a row that is not byte-exact stores 0 and raises the status bit."""
    from prism_amd import _native as N
    for shape in ((10, 10, 1), (6,)):
        buf = _buffer(dev, "uint8")
        st = OC.Streams(shape, N_STREAMS, seed=2).step()
        _put(buf, st)                                                 # (allocates; rows 0 .. 7)
        O = buf.obs_elems
        rows = np.random.default_rng(3).choice(OC.BYTE_VALUES, size=(4, 2, O)).astype(np.float32)
        for bad, status in ((None, 0), (0.5, N.STATUS_OBS_INEXACT)):
            if bad is not None:
                rows[2, 0, 1] = bad
            d = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(dev)
            slots, prev = d(np.arange(8, 12, dtype=np.int32)), d(np.full(4, -1, np.int32))
            obs, succ = d(rows[:, 0]), d(rows[:, 1])
            reward, action, flags = d(np.zeros(4, np.float32)), d(np.zeros(4, np.int32)), d(np.full(4, 4, np.uint8))
            buf._call("prism_replay_insert_ring", N.RING_U8, 4, N.ptr(slots), N.ptr(obs), N.ptr(succ), N.OBS_F32, N.ptr(reward),
                      N.ptr(action), N.ptr(flags), N.ptr(prev), 0.5, 1e-8)
            torch.cuda.synchronize()
            want = OC.narrow(rows)[0]
            np.testing.assert_array_equal(buf.obs[8:12].cpu().numpy(), want[:, 0])
            np.testing.assert_array_equal(buf.succ_obs[8:12].cpu().numpy(), want[:, 1])
            assert int(buf.status.item()) == status


# ---------------------------------------------------------------------------------------------- 8. old against new
def _through_the_ring_entry_points(buf):
    """An fp32 buffer whose native calls go through the prism_*_ring entry points with PRISM_RING_F32."""
    from prism_amd import _native as N
    real = buf._call

    def call(name, *a, **kw):
        if name == "prism_replay_insert":                             # (n, slots, obs, succ | reward .. prev, alpha, eps)
            return real("prism_replay_insert_ring", N.RING_F32, *a[:4], N.OBS_F32, *a[4:], **kw)
        if name == "prism_replay_ingest":
            return real("prism_replay_ingest_ring", N.RING_F32, *a, None, **kw)
        if name == "prism_replay_ingest_tracked":
            return real("prism_replay_ingest_ring", N.RING_F32, *a, **kw)
        if name == "prism_replay_gather":
            return real("prism_replay_gather_ring", N.RING_F32, *a, **kw)
        return real(name, *a, **kw)
    buf._call, buf.renamed = call, True
    return buf


@pytest.mark.parametrize("tracked", [False, True])
@pytest.mark.parametrize("shape", [(10, 10, 4), (6,)])
def test_ring_entry_points_of_the_fp32_kind_equal_the_old_ones(dev, shape, tracked):
    kw = dict(reward_clipping_type="dopamine_clamp") if tracked else {}
    old, new = _buffer(dev, "float32", **kw), _through_the_ring_entry_points(_buffer(dev, "float32", **kw))
    if tracked:
        old.track_episodes(), new.track_episodes()
    gen = OC.Streams(shape, N_STREAMS, seed=4)
    steps = [gen.step() for _ in range(7)]
    for k, st in enumerate(steps):
        conv = (lambda x: x) if k % 2 else (lambda x: x.astype(np.float32))          # both staging kinds of ingest
        _put(old, st, conv), _put(new, st, conv)
    _assert_twin(old, new, "ingest")
    if tracked:
        assert old.episode_stats() == new.episode_stats() and old.episode_stats()["rows"] == 56
    extra = [gen.step() for _ in range(2)]
    _extend_rows(old, extra), _extend_rows(new, extra)                # prism_replay_insert
    _assert_twin(old, new, "insert")


def test_front_ring_of_the_fp32_kind_equals_prism_step_front(dev, monkeypatch):
    from prism_amd import _native as N
    case = OC.FUSED_CASES["per_c4_b16"]
    old, new = _learner(dev, case, "float32"), _learner(dev, case, "float32")
    L, seen = N.lib(), []

    def front_ring(ld, rp, *rest):
        seen.append(rest)
        return L.prism_step_front_ring(ld, rp, N.RING_F32, *rest)
    by_old = [_fused_record(old) for _ in range(3)]
    monkeypatch.setattr(L, "prism_step_front", front_ring)
    by_new = [_fused_record(new) for _ in range(3)]
    monkeypatch.undo()
    assert len(seen) == 3
    for k, (a, b) in enumerate(zip(by_old, by_new)):
        for name in a:
            _same(a[name], b[name], f"step {k + 1}: {name}")


# ---------------------------------------------------------------------------------------------- 9. fused step twin
def _learner(dev, case, storage):
    from prism_amd.config import baseline_config
    from prism_amd.learner import Learner
    cfg = baseline_config(2, device=dev, batch_size=case.B, experience_replay_capacity=OC.FUSED_CAPACITY,
                          use_per=case.use_per, n_step_returns_length=OC.FUSED_N_STEP, gamma=0.99)
    cfg.fused_step, cfg.hip_graph, cfg.replay_obs_storage = True, True, storage
    ln = Learner()
    with contextlib.redirect_stdout(io.StringIO()):
        ln.configure(cfg, obs_shape=(10, 10, case.C), n_actions=6)
    orc, prio, obs_b, succ_b = OC.fused_ring(case)
    n, buf = orc.length, ln.experience_buffer
    assert buf.obs_storage == storage
    buf.load_arrays(obs_b[:n].reshape(n, 10, 10, case.C), succ_b[:n], orc.reward[:n], orc.action[:n], orc.flags[:n],
                    orc.link[:n], priorities=prio if case.use_per else None, cursor=orc.cursor)
    return ln


def _fused_record(ln):
    """One fused step; what it sampled, computed and left behind, cloned."""
    buf, agent = ln.experience_buffer, ln.agent
    td = ln.step(timesteps_this_iteration=1)
    torch.cuda.synchronize()
    buf.check_status(), agent.check_status()
    rec = dict(index=buf._index, td=td, loss=agent.out_dl, scalars=agent.scalars, params=agent.flat, **_batch_tensors(buf))
    if buf.use_per:
        rec.update(weight=buf._weight, tree=buf.tree, per_state=buf.per_state)
    return {k: v.clone() for k, v in rec.items()}


@pytest.mark.parametrize("name", list(OC.FUSED_CASES))
def test_fused_step_on_a_byte_ring_equals_the_fp32_twin(dev, name):
    case = OC.FUSED_CASES[name]
    u8, f32 = _learner(dev, case, "uint8"), _learner(dev, case, "float32")
    assert u8.experience_buffer.obs.dtype is torch.uint8 and f32.experience_buffer.obs.dtype is torch.float32
    _same(u8.agent.flat, f32.agent.flat, "initial parameters")
    p0 = u8.agent.flat.clone()
    orc = OC.fused_ring(case)[0]
    sampled = []
    for step in range(1, OC.FUSED_STEPS + 1):
        a, b = _fused_record(u8), _fused_record(f32)
        for k in a:
            _same(a[k], b[k], f"step {step}: {k}")
        sampled += a["index"].tolist()
        if step == 1 or not case.use_per:                             # what the CPU knew ahead (tests/test_obs_ring_host.py)
            known = OC.known_indices(case, u8.experience_buffer.seed)
            assert a["index"].tolist() == known[(step - 1) * case.B:step * case.B].tolist()
        for ln in (u8, f32):
            graphs = [g for g in ln.agent._graphs.values() if isinstance(g, tuple)]
            assert not graphs if not case.full else (graphs or step <= 2), (step, ln.agent._graphs)
    kinds = {OC.successor_class(orc, s) for s in sampled}
    assert kinds == {OC.PRED, OC.NONE, OC.ELSEWHERE}, kinds
    assert not torch.equal(a["params"], p0) and torch.isfinite(a["params"]).all()
    _assert_same_ring(u8.experience_buffer, f32.experience_buffer, "after the steps")


# ---------------------------------------------------------------------------------------------- 10. learn() twin
def _learn(dev, ckpt_dir, storage):
    from prism_amd.collectors import VectorCollector
    from prism_amd.config import baseline_config
    from prism_amd.learner import Learner
    from tests.test_gpu_episodes import ToyEnvs
    cfg = baseline_config(2, device=dev, batch_size=32, experience_replay_capacity=2048, num_initial_random_timesteps=256,
                          timesteps_per_iteration=8, timestep_limit=256 + 8 * 60, timesteps_per_report=80,
                          timesteps_between_evaluations=10 ** 6, target_update_period=40, checkpoint_dir=str(ckpt_dir),
                          log_to_wandb=False, reward_clipping_type="dopamine_clamp")
    cfg.replay_obs_storage = storage
    os.makedirs(ckpt_dir, exist_ok=True)
    envs = ToyEnvs()
    ln = Learner()
    with contextlib.redirect_stdout(io.StringIO()):
        ln.configure(cfg, collector=VectorCollector(envs, cfg))
        buf = ln.experience_buffer
        real_empty, buf.empty = buf.empty, lambda: None               # learn() empties the buffer on exit: keep it
        ln.learn()
        buf.empty = real_empty
    torch.cuda.synchronize()
    return ln


def test_learn_on_a_byte_ring_equals_the_fp32_run(dev, tmp_path):
    u8, f32 = _learn(dev, tmp_path / "u8", "uint8"), _learn(dev, tmp_path / "f32", "float32")
    assert u8.cumulative_timesteps == f32.cumulative_timesteps == 256 + 8 * 60
    assert u8.cumulative_model_updates == f32.cumulative_model_updates == 60
    assert u8.experience_buffer.obs.dtype is torch.uint8 and f32.experience_buffer.obs.dtype is torch.float32
    _same(u8.agent.flat, f32.agent.flat, "final parameters")
    _assert_same_ring(u8.experience_buffer, f32.experience_buffer, "final ring")
    assert u8.experience_buffer.episode_stats() == f32.experience_buffer.episode_stats()
    assert len(u8.experience_buffer) == 256 + 8 * 60 and u8.experience_buffer.obs.any()


# ---------------------------------------------------------------------------------------------- 11. resume across kinds
def _run_step(buf, st, k):
    """One step of a stand-in loop: a collector call, a sample, a priority writeback that depends on what was sampled."""
    _put(buf, st)
    _, info = buf.sample(return_info=True)
    rec = {k_: v.clone() for k_, v in _batch_tensors(buf).items()}
    rec["index"] = info["index"].clone()
    if buf.use_per:
        rec["weight"] = info["_weight"].clone()
        buf.update_priority(info["index"], ((info["index"] * 7 + k) % 13).float() * 0.25 + 0.125)
    return rec


@pytest.mark.parametrize("use_per", [True, False])
def test_snapshots_interchange_between_the_kinds(dev, tmp_path, use_per):
    gen = OC.Streams((10, 10, 4), N_STREAMS, seed=21)
    steps = [gen.step() for _ in range(11)]
    run = _buffer(dev, "uint8", use_per=use_per)
    for k in range(6):
        _run_step(run, steps[k], k)
    snap = run.save_state(tmp_path / "snap")
    part = run._state_part()
    assert part["obs_dtype"] == "uint8" and part["obs"].dtype is torch.uint8
    want = [_run_step(run, steps[k], k) for k in range(6, 11)]
    resumed = {}
    for storage in ("uint8", "float32"):
        buf = resumed[storage] = _buffer(dev, storage, use_per=use_per)
        buf.load_state(snap)
        assert buf.obs.dtype is (torch.uint8 if storage == "uint8" else torch.float32)
        for k, rec in zip(range(6, 11), want):
            got = _run_step(buf, steps[k], k)
            for name in rec:
                _same(got[name], rec[name], f"{storage} ring, step {k}: {name}")
        _assert_same_ring(buf, run, f"{storage} ring after the resumed steps")
    # an fp32 snapshot goes into a byte ring as well ...
    snap32 = resumed["float32"].save_state(tmp_path / "snap32")
    back = _buffer(dev, "uint8", use_per=use_per)
    back.load_state(snap32)
    _assert_same_ring(back, run, "byte ring from the fp32 ring's snapshot")
    # ... unless it holds a value a byte cannot: refused, nothing touched
    spoiled = _buffer(dev, "float32", use_per=use_per)
    spoiled.load_state(snap32)
    spoiled.succ_obs[3, 7] = 0.5
    bad = spoiled.save_state(tmp_path / "bad")
    image = _ring_image(back)
    with pytest.raises(ValueError, match="byte-exact"):
        back.load_state(bad)
    _assert_untouched(back, image)
    # save(): the reference's file, byte for byte the same from either kind; load() brings it back into either
    for storage, buf in resumed.items():
        buf.save(str(tmp_path / f"saved_{storage}"))
    pkl = [open(tmp_path / f"saved_{s}" / "experience_buffer" / "timesteps.pkl", "rb").read() for s in resumed]
    assert pkl[0] == pkl[1] and len(pkl[0]) > 1000
    loaded = []
    for src, storage in itertools.product(resumed, ("uint8", "float32")):
        buf = _buffer(dev, storage, use_per=use_per)
        buf.load(str(tmp_path / f"saved_{src}"))
        assert len(buf) == len(run) and buf.obs.dtype is (torch.uint8 if storage == "uint8" else torch.float32)
        loaded.append(buf)
    for buf in loaded[1:]:
        _assert_same_ring(buf, loaded[0], "load()")
    assert loaded[0].obs.any() and os.path.exists(tmp_path / "saved_uint8" / "experience_buffer" / "hip_sampler.pt")
