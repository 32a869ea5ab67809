"""GPU: exact resume.  ``save_state`` / ``load_state`` of ``HipReplayBuffer``, ``HipAgent`` and ``Learner``, the backup
checkpoint of ``Checkpointer`` and the resume path of ``Learner.learn()``.

The bar is bit-for-bit equality with the uninterrupted run (the twin pattern): run A does 2K iterations; run B does K,
``save_state``, builds FRESH objects, ``load_state``, then K more.  Compared after every iteration: the actions, the TD
errors, the step's scalars; at the end: parameters, optimizer, every row of every ring array, every tree node, the host
mirrors, the three counter totals, the selector and loop state (tests/resume_helpers.py ``full_state``).  Each case is cut
once before the ring is full (eager fused steps) and once after it has been full for several steps (a captured graph
replaying on one side of the cut, warm-up and capture on the other)."""
import contextlib
import io
import os
import subprocess
import sys
import weakref

import numpy as np
import pytest
import torch

from tests import resume_helpers as R

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K_EARLY, K_LATE = 8, 24          # 5 timesteps an iteration into a ring of 96: full from iteration 20; K_LATE cuts 5 full-ring steps in
TWIN_CASES = ["a_iqn_per_egreedy_adam", "b_ids_sampled_full", "c_dqn1_uniform_rmsprop"]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return "cuda:0"


_RUN_A = {}


def run_a(case, tmp_factory):
    """The uninterrupted run of a case, computed once and left unchanged: 2 * K_LATE iterations, every iteration's record,
    the full state after 2 * K_EARLY and at the end."""
    if case not in _RUN_A:
        ln, col = R.make_learner(case, tmp_factory.mktemp("run_a"))
        records, states = [], {}
        for i in range(2 * K_LATE):
            records.append(R.iterate(ln, col))
            if i + 1 in (2 * K_EARLY, 2 * K_LATE):
                states[i + 1] = R.full_state(ln, col)
        _RUN_A[case] = (records, states)
    return _RUN_A[case]


def check_records(got, want, first=0):
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        for name, x, y in zip(("actions", "out_td", "scalars"), g, w):
            R.assert_same(x, y, f"iteration {first + i} {name}")


@pytest.mark.parametrize("K", [K_EARLY, K_LATE], ids=["before_full", "graph_replaying"])
@pytest.mark.parametrize("case", TWIN_CASES)
def test_resumed_run_equals_the_uninterrupted_run(dev, tmp_path, tmp_path_factory, case, K):
    records_a, states_a = run_a(case, tmp_path_factory)
    ln, col = R.make_learner(case, tmp_path / "b")
    records = [R.iterate(ln, col) for _ in range(K)]
    buf = ln.experience_buffer
    full = buf._size == buf.capacity
    assert full == (K == K_LATE)
    if full:          # the cut falls on a replaying graph
        assert any(isinstance(g, tuple) for g in ln.agent._graphs.values())
    assert 0 < ln.timesteps_since_target_model_update < R.TARGET_PERIOD or not ln.use_target_network
    snap = ln.save_state(tmp_path / "snap")
    assert sorted(os.listdir(snap)) == ["MANIFEST.json", "agent", "agent_resume.pt", "learner.pt", "replay.pt"]
    ln2, col2 = R.make_learner(case, tmp_path / "c", collector_seed=999)      # (the script's position comes with the snapshot)
    assert ln2.agent is not ln.agent and ln2.experience_buffer._desc is None
    ln2.load_state(snap)
    records += [R.iterate(ln2, col2) for _ in range(K)]
    check_records(records, records_a[:2 * K])
    if ln.use_target_network:          # a target sync lies on both sides of the cut
        assert K * R.N_ENV >= R.TARGET_PERIOD
    R.assert_same(R.full_state(ln2, col2), states_a[2 * K])
    assert int(ln2.experience_buffer.status.item()) == 0
    ln2.agent.check_status()


def test_snapshot_without_restore_changes_nothing(dev, tmp_path, tmp_path_factory):
    case = TWIN_CASES[0]
    records_a, states_a = run_a(case, tmp_path_factory)
    ln, col = R.make_learner(case, tmp_path / "b")
    records = []
    for i in range(2 * K_LATE):
        records.append(R.iterate(ln, col))
        if i + 1 in (3, K_LATE):          # once with a partly filled ring, once under the replaying graph
            ln.save_state(tmp_path / "snap")
    check_records(records, records_a)
    R.assert_same(R.full_state(ln, col), states_a[2 * K_LATE])


def test_agent_and_buffer_snapshots_stand_alone(dev, tmp_path, tmp_path_factory):
    """``HipAgent.save_state`` and ``HipReplayBuffer.save_state`` by themselves (no Learner part): the agent's directory
    keeps the reference's layout beside the resume part."""
    case, K = TWIN_CASES[1], 4
    records_a, _ = run_a(case, tmp_path_factory)
    ln, col = R.make_learner(case, tmp_path / "b")
    for _ in range(K):
        R.iterate(ln, col)
    ln.agent.save_state(tmp_path / "agent_snap")
    ln.experience_buffer.save_state(tmp_path / "replay_snap")
    assert sorted(os.listdir(tmp_path / "agent_snap")) == ["MANIFEST.json", "agent", "agent_resume.pt"]
    assert sorted(os.listdir(tmp_path / "agent_snap" / "agent")) == ["model.pt", "optimizer.pt", "state.pkl", "target_model.pt"]
    assert sorted(os.listdir(tmp_path / "replay_snap")) == ["MANIFEST.json", "replay.pt"]
    ln2, col2 = R.make_learner(case, tmp_path / "c")
    ln2.agent.load_state(tmp_path / "agent_snap")
    ln2.experience_buffer.load_state(tmp_path / "replay_snap")
    col2.load_state_dict(col.state_dict())
    ln2.timesteps_since_target_model_update = ln.timesteps_since_target_model_update
    check_records([R.iterate(ln2, col2) for _ in range(K)], records_a[K:2 * K], first=K)
    # the plain agent/ directory still loads through the reference-format load()
    ln3, _ = R.make_learner(case, tmp_path / "d")
    ln3.agent.load(str(tmp_path / "agent_snap"))
    assert torch.equal(ln3.agent.flat, ln.agent.flat)


def test_parity_modes(dev, tmp_path):
    """``per_mass_rng = "numpy"``, ``tau_rng = "torch"``: the priority masses come from NumPy's global generator, the
    quantile samples from the device's torch generator, the step runs sample() / update() / update_priority() unfused --
    the snapshot carries both generators."""
    case, K = "parity_numpy_torch", 6
    ln, col = R.make_learner(case, tmp_path / "a")
    assert not ln.fused
    records_a = [R.iterate(ln, col) for _ in range(2 * K)]
    state_a = R.full_state(ln, col)
    ln, col = R.make_learner(case, tmp_path / "b")
    records = [R.iterate(ln, col) for _ in range(K)]
    snap = ln.save_state(tmp_path / "snap")
    np.random.seed(1)                         # whatever the process did in between must not matter
    torch.manual_seed(1)
    ln2, col2 = R.make_learner(case, tmp_path / "c", collector_seed=5)
    ln2.load_state(snap)
    records += [R.iterate(ln2, col2) for _ in range(K)]
    check_records(records, records_a)
    R.assert_same(R.full_state(ln2, col2), state_a)
    assert state_a["tau_draws"] > 0 and state_a["per_draws"] == 2 * K * R.BATCH


def test_fresh_process(dev, tmp_path):
    """The parent saves and goes on; a child process (started fresh: nothing is exec'ed in a process that has touched the
    GPU) loads the snapshot, runs the same K iterations and leaves its records and final state in a file."""
    case, K = TWIN_CASES[0], K_LATE
    ln, col = R.make_learner(case, tmp_path / "b")
    for _ in range(K):
        R.iterate(ln, col)
    snap = ln.save_state(tmp_path / "snap")
    out = tmp_path / "child.pt"
    res = subprocess.run([sys.executable, "-m", "tests.resume_helpers", case, str(snap), str(K), str(out), str(tmp_path / "child")],
                         cwd=ROOT, timeout=120, capture_output=True, text=True)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    records = [R.iterate(ln, col) for _ in range(K)]
    child = torch.load(out, weights_only=True)
    check_records([tuple(r) for r in child["records"]], records, first=K)
    R.assert_same(child["state"], R.full_state(ln, col))


# ---------------------------------------------------------------------- Learner.learn() and the backup checkpoint
def _learn(case, ckpt_dir, limit, resume=False, raise_limit_to=None, **over):
    ln, col = R.make_learner(case, ckpt_dir, timestep_limit=limit, **over)
    buf = ln.experience_buffer
    with contextlib.redirect_stdout(io.StringIO()):
        if resume:
            latest = ln.checkpointer.latest_backup()
            assert latest is not None
            ln.load_state(latest)
            ln.timestep_limit = raise_limit_to
        real_empty = buf.empty
        buf.empty = lambda: None              # learn() empties the buffer on exit: keep it for the comparison
        try:
            ln.learn()
        finally:
            buf.empty = real_empty
    return ln, col


def test_learn_resumes_from_the_backup_checkpoint(dev, tmp_path):
    case, L = TWIN_CASES[0], 40 + R.N_ENV * 30          # 40 random timesteps, then 30 iterations: the ring is full, reports happen
    ref, ref_col = _learn(case, tmp_path / "ref", 2 * L, backup_checkpoints=True)
    want = R.full_state(ref, ref_col)
    assert want["cumulative_timesteps"] == 2 * L and want["cumulative_model_updates"] == (2 * L - 40) // R.N_ENV
    first, _ = _learn(case, tmp_path / "run", L, backup_checkpoints=True)
    assert first.cumulative_timesteps == L
    backup = first.checkpointer.latest_backup()
    assert backup == os.path.join(first.checkpointer.save_dir, "backup_checkpoint") and os.path.isfile(os.path.join(backup, "MANIFEST.json"))
    second, col = _learn(case, tmp_path / "run", L, resume=True, raise_limit_to=2 * L, backup_checkpoints=True)
    assert col.closed and second.agent is not first.agent
    R.assert_same(R.full_state(second, col), want)
    # the agent checkpoints of the two legs together are those of the one run; the way out rotated the backup in place
    names = lambda ln: sorted(d for d in os.listdir(ln.checkpointer.save_dir) if d.startswith("agent_checkpoint_"))
    assert names(second) == names(ref) and len(names(ref)) > 2
    assert second.checkpointer.latest_backup() == backup and not os.path.exists(backup + ".prev")
    from prism_amd.util import snapshot
    assert snapshot.read_snapshot(backup, ["learner"])[0]["learner"]["cumulative_timesteps"] == 2 * L


def test_backup_checkpoints_are_off_by_default_and_never_mask_an_error(dev, tmp_path):
    case = TWIN_CASES[2]
    ln, _ = _learn(case, tmp_path / "off", 60)
    assert ln.checkpointer.latest_backup() is None
    assert not os.path.exists(os.path.join(ln.checkpointer.save_dir, "backup_checkpoint"))
    # the loop dies AND the snapshot on the way out fails: the loop's error is the one that surfaces
    ln, col = R.make_learner(case, tmp_path / "err", timestep_limit=60, backup_checkpoints=True)

    def broken_step(*a, **k):
        raise ZeroDivisionError("the loop's own error")

    def broken_snapshot(path):
        raise OSError("disk full")
    ln.step, ln.save_state = broken_step, broken_snapshot
    with contextlib.redirect_stdout(io.StringIO()), pytest.warns(UserWarning, match="backup checkpoint"):
        with pytest.raises(ZeroDivisionError):
            ln.learn()
    assert col.closed and len(ln.experience_buffer) == 0          # the rest of the way out still ran


# ---------------------------------------------------------------------- refusals
@pytest.mark.parametrize("field,over", [("capacity", dict(experience_replay_capacity=128)),
                                        ("n_step", dict(n_step_returns_length=1)),
                                        ("n_actions", dict(n_actions=5)),
                                        ("iqn_width", dict(iqn_quantile_model_feature_dim=256)),
                                        ("optimizer_kind", dict(use_adam=False, use_rmsprop=True))])
def test_mismatches_are_refused_before_anything_is_touched(dev, tmp_path, tmp_path_factory, field, over):
    case = TWIN_CASES[0]
    if "snap" not in _REFUSAL:
        ln, col = R.make_learner(case, tmp_path_factory.mktemp("refusal"))
        for _ in range(2):
            R.iterate(ln, col)
        _REFUSAL["snap"] = ln.save_state(tmp_path_factory.mktemp("refusal_snap") / "snap")
        _REFUSAL["stored"] = dict(capacity=96, n_step=3, n_actions=6, iqn_width=128, optimizer_kind=0)
    other, col = R.make_learner(case, tmp_path / "other", **over)
    agent, buf = other.agent, other.experience_buffer
    flat0, eps0 = agent.flat.clone(), agent.action_selector.epsilon.get_state()
    np_state = np.random.get_state()[1].copy()
    with pytest.raises(ValueError) as e:
        other.load_state(_REFUSAL["snap"])
    current = {"capacity": 128, "n_step": 1, "n_actions": 5, "iqn_width": 256, "optimizer_kind": 1}[field]
    msg = str(e.value)
    assert field in msg and repr(_REFUSAL["stored"][field]) in msg and repr(current) in msg
    assert torch.equal(agent.flat, flat0) and agent.n_updates == 0 and agent._act_draws == 0
    assert agent.action_selector.epsilon.get_state() == eps0 and int(agent.optimizer.step_t.item()) == 0
    assert buf._desc is None and len(buf) == 0 and buf._draws == 0 and col.obs is None
    assert other.cumulative_model_updates == 0 and not other._resumed
    np.testing.assert_array_equal(np.random.get_state()[1], np_state)


_REFUSAL = {}


# ---------------------------------------------------------------------- buffer level
RING = ("obs", "succ_obs", "reward", "action", "flags", "link", "back", "tree", "per_state", "status")


def _buffer(dev, capacity=24, batch=4, use_per=True, **kw):
    from prism_amd.experience import HipReplayBuffer
    return HipReplayBuffer(capacity, batch, device=dev, n_step=3, gamma=0.99, use_per=use_per, alpha=0.5, beta=0.5, seed=5, **kw)


def _ring(buf):
    buf.flush()
    torch.cuda.synchronize()
    st = {k: getattr(buf, k).cpu().clone() for k in RING if getattr(buf, k) is not None}
    st.update(slot_id=torch.from_numpy(buf._slot_id.copy()), size=buf._size, cursor=buf.buffer._writer._cursor,
              serial=buf._serial, draws=buf._draws + buf._fused_draws,
              pending=sorted([int(k), int(v[0]), int(v[1])] for k, v in buf._pending.items()),
              stream_tab=None if buf._stream_tab is None else buf._stream_tab.cpu().clone())
    return st


def _vec_step(rng, n, open_=False, shape=(10, 10, 4)):
    done = np.zeros(n, bool) if open_ else rng.random_sample(n) < 0.15
    trunc = np.zeros(n, bool) if open_ else ~done & (rng.random_sample(n) < 0.1)
    return dict(obs=rng.random_sample((n,) + shape) < 0.2, next_obs=rng.random_sample((n,) + shape) < 0.2,
                action=rng.randint(0, 6, n).astype(np.int32), reward=rng.standard_normal(n).astype(np.float32),
                done=done, truncated=trunc)


def test_buffer_cut_with_staged_rows_a_pending_entry_and_an_open_chain(dev, tmp_path):
    """The cut falls where ``save()`` (the reference's format) loses the most: rows staged by ``extend()`` and not yet
    flushed, a live ``_pending`` entry whose successor arrives after the restore, open rows of three ``extend_batch``
    streams.  The successor links exactly as in the twin that was never cut, and so does everything after it."""
    from prism_amd.experience import Timestep
    rng = np.random.RandomState(2)
    chain = [Timestep(id=100 + i, obs=torch.from_numpy((rng.random_sample((10, 10, 4)) < 0.2).astype(np.float32)))
             for i in range(12)]
    for i, t in enumerate(chain[:-1]):
        t.reward, t.action, t.done, t.truncated = float(np.float32(rng.standard_normal())), int(rng.randint(6)), i == 7, False
        if not t.done:
            t.next = weakref.ref(chain[i + 1])
    vec = [_vec_step(rng, 3, open_=(k in (1, 2))) for k in range(9)]
    idx, pr = torch.tensor([0, 2, 4], device=dev), torch.tensor([0.3, 2.5, 1.1], device=dev)
    ops = [lambda b: b.extend_batch(**vec[0]), lambda b: b.extend(chain[0]), lambda b: b.extend(chain[1]),
           lambda b: b.extend_batch(**vec[1]), lambda b: b.update_priority(idx, pr), lambda b: b.sample(),
           lambda b: b.extend(chain[2]), lambda b: b.extend(chain[3])]
    cut = len(ops)
    ops += [lambda b: b.extend(chain[4]), lambda b: b.extend_batch(**vec[2])]
    ops += [op for k in range(3, 9) for op in (lambda b, k=k: b.extend_batch(**vec[k]), lambda b, k=k: b.extend(chain[k + 2]),
                                                lambda b: b.sample())]
    twin, buf = _buffer(dev), _buffer(dev)
    for op in ops:
        op(twin)
    for op in ops[:cut]:
        op(buf)
    assert buf._n_staged == 2 and list(buf._pending) == [chain[4].id]          # staged rows and a live pending entry at the cut
    open_slot = buf._pending[chain[4].id][0]
    snap = buf.save_state(tmp_path / "snap")
    new = _buffer(dev)
    new.load_state(snap)
    assert new._n_staged == 0 and new._pending == buf._pending and int(new.link[open_slot]) == -1
    R.assert_same(_ring(new), _ring(buf))
    succ_slot = new.buffer._writer._cursor
    for op in ops[cut:]:
        op(new)
    got, want = _ring(new), _ring(twin)
    R.assert_same(got, want)
    assert twin._size == twin.capacity and twin._serial > twin.capacity                  # the ring wrapped after the cut
    # the first sample after the restore: same indices, weights and batch (the draw count travelled)
    new2 = _buffer(dev)
    new2.load_state(snap)
    b0, i0 = buf.sample(return_info=True)
    b1, i1 = new2.sample(return_info=True)
    torch.cuda.synchronize()
    R.assert_same({k: v.cpu() for k, v in i1.items()}, {k: v.cpu() for k, v in i0.items()})
    R.assert_same(b1["next"]["observation"].cpu(), b0["next"]["observation"].cpu())
    # and the successor that arrived after the restore linked to the row that was open at the cut
    new3 = _buffer(dev)
    new3.load_state(snap)
    new3.extend(chain[4])
    new3.flush()
    assert int(new3.link[open_slot]) == succ_slot and int(new3.back[succ_slot]) == open_slot


@pytest.mark.parametrize("kind", ["binary", "bytes", "fractions", "negative_zero", "above_255"])
def test_observations_take_the_narrowest_exact_form(dev, tmp_path, kind):
    from prism_amd.util import snapshot
    rng = np.random.RandomState(4)
    n, shape = 6, (10, 10, 4)
    if kind == "binary":
        mk = lambda: (rng.random_sample((n,) + shape) < 0.2).astype(np.float32)
    elif kind == "bytes":
        mk = lambda: rng.randint(0, 256, (n,) + shape).astype(np.float32)
    else:
        mk = lambda: rng.random_sample((n,) + shape).astype(np.float32)
    steps = [dict(_vec_step(rng, n, open_=True), obs=mk(), next_obs=mk()) for _ in range(2)]
    if kind == "negative_zero":
        for s in steps:
            s["obs"], s["next_obs"] = np.round(s["obs"]), np.round(s["next_obs"])
        steps[1]["next_obs"][3, 2, 1, 0] = -0.0                # every value an integer in [0, 255], one of them -0.0
    if kind == "above_255":
        for s in steps:
            s["obs"], s["next_obs"] = np.round(s["obs"]), np.round(s["next_obs"])
        steps[0]["obs"][5, 9, 9, 3] = 256.0
    buf = _buffer(dev, capacity=16)
    for s in steps:
        buf.extend_batch(**s)
    snap = buf.save_state(tmp_path / "snap")
    part = snapshot.read_snapshot(snap)[0]["replay"]
    want = torch.uint8 if kind in ("binary", "bytes") else torch.float32
    assert part["obs"].dtype == part["succ_obs"].dtype == want and part["obs_dtype"] == str(want).split(".")[1]
    assert part["rows"] == 2 * n and part["obs"].shape == (2 * n, 400)
    new = _buffer(dev, capacity=16)
    new.load_state(snap)
    R.assert_same(_ring(new), _ring(buf))
    if kind == "negative_zero":
        assert int(new.succ_obs.view(torch.int32).min()) == -(2 ** 31)          # the sign bit came back


def test_uniform_replay_and_rows_behind_size(dev, tmp_path):
    """No trees (uniform replay); and a ring a reference-format load() filled keeps link-target rows BEHIND its size:
    they are rows of the snapshot too."""
    rng = np.random.RandomState(6)
    buf = _buffer(dev, use_per=False)
    for k in range(5):
        buf.extend_batch(**_vec_step(rng, 3, open_=(k == 4)))
    buf.save(str(tmp_path / "ref"))
    loaded = _buffer(dev, use_per=False)
    loaded.load(str(tmp_path / "ref"))
    snap = loaded.save_state(tmp_path / "snap")
    new = _buffer(dev, use_per=False)
    new.load_state(snap)
    R.assert_same(_ring(new), _ring(loaded))
    assert new.tree is None and len(new) == len(loaded)
    from prism_amd.util import snapshot
    assert snapshot.read_snapshot(snap)[0]["replay"]["rows"] == loaded._valid_rows() >= len(loaded)
    with pytest.raises(ValueError, match="use_per"):
        _buffer(dev, use_per=True).load_state(snap)
    with pytest.raises(ValueError, match="mass_rng"):
        _buffer(dev, use_per=False, mass_rng="numpy").load_state(snap)


def test_keep_streams_false_closes_every_stream(dev, tmp_path):
    rng = np.random.RandomState(8)
    buf = _buffer(dev)
    for _ in range(3):
        buf.extend_batch(**_vec_step(rng, 4, open_=True))
    snap = buf.save_state(tmp_path / "snap")
    nxt = _vec_step(rng, 4, open_=True)
    kept, closed = _buffer(dev), _buffer(dev)
    kept.load_state(snap)
    closed.load_state(snap, keep_streams=False)
    assert int((closed._stream_tab >= 0).sum()) == 0 and closed._pending == {} and closed._serial == closed.buffer._writer._cursor
    first = kept.extend_batch(**nxt)
    assert closed.extend_batch(**nxt) == first == 12
    torch.cuda.synchronize()
    rows = slice(first, first + 4)
    assert kept.back[rows].tolist() == [8, 9, 10, 11] and kept.link[8:12].tolist() == [12, 13, 14, 15]
    assert closed.back[rows].tolist() == [-1] * 4 and closed.link[8:12].tolist() == [-1] * 4          # unlinked
    for name in ("obs", "reward", "action"):                                                  # same rows otherwise
        assert torch.equal(getattr(kept, name), getattr(closed, name)), name
    closed.extend_batch(**_vec_step(rng, 4, open_=True))                                                  # and the streams go on
    torch.cuda.synchronize()
    assert closed.back[16:20].tolist() == [12, 13, 14, 15]
    closed.check_status()
