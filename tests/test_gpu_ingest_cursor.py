"""``prism_replay_ingest_cursor`` on the GPU: a ring fed through the device cursor (alternating slots) against a twin fed by
``extend_batch``, bit for bit; the two launches captured into one hipGraph and replayed; a negative cursor.

Shapes: those of tests/resume_helpers.py (capacity 96, N = 5, C = 4), which put the wrap inside a call."""
import pytest
import torch

from tests import resume_helpers as RH

pytestmark = pytest.mark.gpu

CAP, SHAPE = RH.CAPACITY, (10, 10, RH.C)
SIZES = (1, 3, 5, 64, 65)          # on capacity 96: a wrap inside a call (64, 65) and a call that overwrites its predecessors' slots


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return "cuda:0"


def _buffer(dev, storage, tracked, use_per=True):
    from prism_amd.experience import HipReplayBuffer
    buf = HipReplayBuffer(CAP, RH.BATCH, device=dev, n_step=3, gamma=0.99, use_per=use_per, seed=11, obs_storage=storage,
                          reward_clipping_type="dopamine_clamp" if tracked else None)
    if tracked:
        buf.track_episodes(0.9)
    buf.reserve_streams(max(SIZES))
    return buf


def _rows(gen, n, kind, dev):
    """One call's transitions as device tensors of the dtypes the cursor form takes in place: boolean planes as float32 or
    uint8, rewards beyond [-1, 1] (the clamp acts), episode ends and truncations (both at once happens too)."""
    planes = lambda: (torch.rand((n,) + SHAPE, generator=gen) < 0.3).to(torch.float32 if kind == "f32" else torch.uint8)
    rows = dict(obs=planes(), next_obs=planes(), action=torch.randint(0, RH.A, (n,), generator=gen, dtype=torch.int32),
                reward=2.0 * torch.randn(n, generator=gen), done=(torch.rand(n, generator=gen) < 0.12).to(torch.uint8),
                truncated=(torch.rand(n, generator=gen) < 0.06).to(torch.uint8))
    return {k: v.to(dev) for k, v in rows.items()}


def _state(buf):
    torch.cuda.synchronize()
    st = {name: getattr(buf, name).cpu().clone() for name in ("obs", "succ_obs", "reward", "action", "flags", "link", "back",
                                                              "tree", "per_state", "status") if getattr(buf, name) is not None}
    st["stream_tab"] = buf._stream_tab.cpu().clone()
    if buf._ep is not None:
        st.update(ep_return=buf._ep_return.cpu().clone(), ep_length=buf._ep_length.cpu().clone(),
                  ep_words=buf._ep_words.cpu().clone())
    st["mirrors"] = [int(buf.buffer._writer._cursor), int(buf._serial), int(buf._size)]
    st["slot_id"] = torch.from_numpy(buf._slot_id.copy())
    return st


def _eager(buf, r):
    return buf.extend_batch(r["obs"], r["next_obs"], r["action"], r["reward"], r["done"], r["truncated"])


def _cursor(buf, slot, r):
    buf.enqueue_extend_cursor(slot, r["obs"], r["next_obs"], r["action"], r["reward"], r["done"], r["truncated"])


@pytest.mark.parametrize("tracked", [False, True])
@pytest.mark.parametrize("storage", ["float32", "uint8"])
def test_twin_rings_over_40_calls(dev, storage, tracked):
    gen = torch.Generator().manual_seed(5)
    a, b = _buffer(dev, storage, tracked), _buffer(dev, storage, tracked)
    first = _rows(gen, RH.N_ENV, "f32", dev)          # an eager call on both: the ring exists, and the cursor has to be seeded
    _eager(a, first), _eager(b, first)
    slot = 0
    a.seed_cursor(slot)
    for call in range(40):
        n = SIZES[call % len(SIZES)]
        r = _rows(gen, n, "u8" if (call // len(SIZES)) & 1 else "f32", dev)
        before = a._serial
        assert _eager(b, r) == before % CAP
        a.seed_cursor(slot)                            # (a no-op: the host knows what the last launch left)
        _cursor(a, slot, r)
        assert a.extend_cursor_mirror(n, slot) == before % CAP
        words = a._cursor_words.cpu().tolist()
        assert words[slot] == before and words[slot ^ 1] == before + n == a._serial, (call, words)
        slot ^= 1
        if call % 10 == 9:
            RH.assert_same(_state(a), _state(b), f"after call {call}")
    assert a._serial == RH.N_ENV + 8 * sum(SIZES) and len(a) == CAP
    assert int(a.status.item()) == 0
    if tracked:
        assert a.episode_stats() == b.episode_stats() and a.episode_stats()["episodes"] > 20
    # an eager call moves the count behind the cursor's back: the next cursor launch is seeded again
    r = _rows(gen, 3, "f32", dev)
    _eager(a, r), _eager(b, r)
    r = _rows(gen, 5, "f32", dev)
    _eager(b, r)
    a.seed_cursor(slot)
    _cursor(a, slot, r)
    a.extend_cursor_mirror(5, slot)
    RH.assert_same(_state(a), _state(b), "after an eager call in between")


@pytest.mark.parametrize("storage,tracked", [("float32", True), ("uint8", False)])
def test_two_launches_in_one_graph_replayed_25_times(dev, storage, tracked):
    from prism_amd.agents.hip_agent import graph_capture
    gen = torch.Generator().manual_seed(9)
    a, b = _buffer(dev, storage, tracked), _buffer(dev, storage, tracked)
    kind = "u8" if storage == "uint8" else "f32"
    n0, n1 = 5, 64                                     # 69 rows a replay on 96 slots: every second replay wraps inside a launch
    x0, x1 = _rows(gen, n0, kind, dev), _rows(gen, n1, kind, dev)

    def fresh():
        for x, n in ((x0, n0), (x1, n1)):
            for k, v in _rows(gen, n, kind, dev).items():
                x[k].copy_(v)                          # the captured launches read these addresses: rewritten in place

    def twin():
        _eager(b, x0), _eager(b, x1)

    _eager(a, x0), _eager(a, x1)                       # first eagerly (the ring exists) ...
    twin()
    a.seed_cursor(0)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with graph_capture(g):                             # ... then capture: a slot-0 and a slot-1 launch, one chain
        _cursor(a, 0, x0)
        _cursor(a, 1, x1)
    for replay in range(25):
        fresh()
        before = a._serial
        g.replay()
        a.extend_cursor_mirror(n0, 0)
        a.extend_cursor_mirror(n1, 1)
        twin()
        if replay % 8 == 7 or replay == 24:
            RH.assert_same(_state(a), _state(b), f"after replay {replay}")
            assert a._cursor_words.cpu().tolist() == [before + n0 + n1, before + n0]
    assert a._serial == 26 * (n0 + n1) and int(a.status.item()) == 0


def test_negative_cursor_writes_nothing_and_raises(dev):
    from prism_amd import _native as N
    gen = torch.Generator().manual_seed(3)
    buf = _buffer(dev, "float32", True)
    for _ in range(3):
        _eager(buf, _rows(gen, RH.N_ENV, "f32", dev))
    buf.seed_cursor(0)
    buf._cursor_words[0] = -7                           # what no host check can see
    buf._cursor_words[1] = 123
    want = _state(buf)
    _cursor(buf, 0, _rows(gen, RH.N_ENV, "f32", dev))
    got = _state(buf)
    assert buf._cursor_words.cpu().tolist() == [-7, -7]          # passed on unchanged
    assert int(got["status"].item()) == N.STATUS_INGEST_BAD_CURSOR == 16
    want["status"] = got["status"]
    RH.assert_same(got, want, "a refused launch")
    with pytest.raises(RuntimeError, match="negative ring cursor"):
        buf.check_status()
