"""GPU: ``prism_step_front_cursor`` -- the fused step's front launch with the ring's size read from the device -- against the
by-value ``prism_step_front_ring`` on twin rings and twin workspaces, bit for bit: what it sampled, the whole static batch,
the whole workspace (both embeddings, the sibling record, the ticket words), p_sum / p_min and the status word.

Shapes: those of tests/resume_helpers.py (capacity 96, tree capacity 128; B = 16) and B = 272 for the split writeback.  The
ring holds 96 rows of three interleaved streams at n_step = 3, gamma = 0.99 (tests/replay_cases.py): most walks take two
hops, which is what holds the cursor kernels' argument layout to the body's by-offset read of ``gammas``.  A size below 96 is
only ever an argument here: both launches sample the same prefix of the same ring."""
import contextlib
import ctypes
import io

import numpy as np
import pytest
import torch

from tests import replay_cases as R

pytestmark = pytest.mark.gpu

CAP = 96
WORDS = (1, 2, CAP // 2 + 1, CAP - 1, CAP, CAP + 7)          # the last reads as CAP
RING = ("obs", "succ_obs", "reward", "action", "flags", "link", "back", "tree")
BATCH = ("_obs", "_next_obs", "_reward", "_gamma", "_nonterminal", "_action")


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return "cuda:0"


_TWINS = {}


def _learner(dev, case, storage):
    from prism_amd.config import baseline_config
    from prism_amd.learner import Learner
    cfg = baseline_config(2, device=dev, batch_size=case.B, experience_replay_capacity=case.capacity, use_per=case.use_per,
                          n_step_returns_length=case.n_step, gamma=case.gamma)
    cfg.fused_step, cfg.hip_graph, cfg.replay_obs_storage = True, True, storage
    ln = Learner()
    with contextlib.redirect_stdout(io.StringIO()):
        ln.configure(cfg, obs_shape=(10, 10, case.C), n_actions=6)
    orc, prio = R.build_ring(case)
    n, buf = orc.length, ln.experience_buffer
    assert n == CAP
    buf.load_arrays(orc.obs[:n].reshape(n, 10, 10, case.C), orc.succ_obs[:n], orc.reward[:n], orc.action[:n], orc.flags[:n],
                    orc.link[:n], priorities=prio if case.use_per else None, cursor=orc.cursor)
    buf.seed_cursor(0)                                          # (allocates the two cursor words)
    if buf._index is None or buf._index.shape[0] != case.B:
        buf._alloc_batch(case.B)
    torch.cuda.synchronize()
    return ln


def _twins(dev, use_per=True, storage="float32", B=16, C=4):
    """(by-value learner, cursor learner) of one configuration: same seed, same ring; built once per module."""
    key = (use_per, storage, B, C)
    if key not in _TWINS:
        case = R._case(CAP, CAP, C=C, B=B, use_per=use_per, seed=900 + C + B)
        _TWINS[key] = (_learner(dev, case, storage), _learner(dev, case, storage))
        a, b = _TWINS[key]
        assert torch.equal(a.agent.flat, b.agent.flat)
        assert a.experience_buffer._ring_kind == b.experience_buffer._ring_kind == (1 if storage == "uint8" else 0)
    return _TWINS[key]


def _front(ln, size=None, slot=None):
    """The front launch alone, on the learner's own descriptor: by value (``size``) or reading ``cursor[slot]``."""
    from prism_amd import _native as N
    agent, buf = ln.agent, ln.experience_buffer
    L, st = N.lib(), N.current_stream_handle
    d = agent._fused_begin(buf)
    rp, beta = ctypes.byref(buf._desc), 0.5
    with torch.cuda.device(agent.device):
        if slot is None:
            N.check(L.prism_step_front_ring(ctypes.byref(d), rp, buf._ring_kind, size, None, buf.seed, buf._draws, beta,
                                            N.ptr(buf._index), N.ptr(buf._weight), st()), "prism_step_front_ring")
        else:
            N.check(L.prism_step_front_cursor(ctypes.byref(d), rp, buf._ring_kind, N.ptr(buf._cursor_words), slot, None,
                                              buf.seed, buf._draws, beta, N.ptr(buf._index), N.ptr(buf._weight), st()),
                    "prism_step_front_cursor")


def _record(ln):
    torch.cuda.synchronize()
    agent, buf = ln.agent, ln.experience_buffer
    rec = {k: getattr(buf, k).clone() for k in BATCH}
    rec.update(index=buf._index.clone(), workspace=agent.workspace.clone().view(torch.int32), status=buf.status.clone())
    if buf.use_per:
        rec.update(weight=buf._weight.clone(), per_state=buf.per_state[1:3].clone())
    return rec


def _ring(ln):
    buf = ln.experience_buffer
    return {k: getattr(buf, k).clone() for k in RING if getattr(buf, k) is not None}


def _same(a, b, where):
    assert a.keys() == b.keys(), where
    for k in a:
        x, y = a[k], b[k]
        assert x.dtype == y.dtype and x.shape == y.shape, f"{where}: {k}"
        if x.dtype.is_floating_point:
            x, y = x.contiguous().view(torch.int32), y.contiguous().view(torch.int32)
        assert torch.equal(x, y), f"{where}: {k}: {int((x != y).sum())} of {x.numel()} values differ"


def _compare(dev, word, slot, **kw):
    val, cur = _twins(dev, **kw)
    buf = cur.experience_buffer
    before = _ring(cur)
    buf._cursor_words[slot] = word
    buf._cursor_words[slot ^ 1] = 3 if word != 3 else 5          # the other word is not the one that is read
    _front(val, size=min(word, CAP))
    _front(cur, slot=slot)
    want, got = _record(val), _record(cur)
    _same(got, want, f"word {word} in slot {slot} ({kw})")
    assert int(got["status"].item()) == 0
    assert int(got["index"].min()) >= 0 and int(got["index"].max()) < min(word, CAP)
    _same(_ring(cur), before, "the ring after the launch")
    assert buf._cursor_words.tolist() == ([word, 3 if word != 3 else 5] if slot == 0 else [3 if word != 3 else 5, word])
    return got


@pytest.mark.parametrize("slot", [0, 1])
@pytest.mark.parametrize("word", WORDS)
def test_prioritized_fp32_ring_every_word_both_slots(dev, word, slot):
    got = _compare(dev, word, slot)
    if word >= CAP - 1:
        # n_step = 3: walks of three rewards were sampled, each hop's gamma read from the argument segment by offset
        gam = got["_gamma"].cpu().numpy().ravel().astype(np.float64)
        assert (np.abs(gam - 0.99 ** 3) < 1e-6).any() and len(set(got["index"].tolist())) > 4


@pytest.mark.parametrize("word", WORDS)
def test_uniform_replay_every_word(dev, word):
    _compare(dev, word, word & 1, use_per=False)


@pytest.mark.parametrize("use_per", [True, False])
@pytest.mark.parametrize("word", WORDS)
def test_byte_ring_every_word(dev, word, use_per):
    _compare(dev, word, (word & 1) ^ 1, use_per=use_per, storage="uint8")


@pytest.mark.parametrize("storage", ["float32", "uint8"])
@pytest.mark.parametrize("word", [2, CAP // 2 + 1, CAP - 1, CAP + 7])
def test_batch_272_past_the_split_writeback(dev, word, storage):
    _compare(dev, word, word & 1, B=272, storage=storage)


@pytest.mark.parametrize("word", [CAP // 2 + 1, CAP])
def test_seven_channels(dev, word):
    _compare(dev, word, 1, C=7)


@pytest.mark.parametrize("kw", [dict(), dict(use_per=False, storage="uint8")], ids=["per_f32", "uniform_u8"])
def test_one_capture_replayed_over_five_sizes(dev, kw):
    from prism_amd.agents.hip_agent import graph_capture
    val, cur = _twins(dev, **kw)
    buf, slot = cur.experience_buffer, 1
    buf._cursor_words[slot] = CAP
    buf._cursor_words[slot ^ 1] = 7
    _front(cur, slot=slot)                                      # (warm: nothing is set up inside the capture)
    _front(val, size=CAP)                                       # (the twins see the same launches in the same order)
    torch.cuda.current_stream().synchronize()
    g = torch.cuda.CUDAGraph()
    with graph_capture(g):
        _front(cur, slot=slot)
    for word in (2, CAP - 1, CAP // 2 + 1, CAP + 7, 1):
        buf._cursor_words[slot] = word                          # rewritten in place: the graph holds the address
        g.replay()
        _front(val, size=min(word, CAP))
        _same(_record(cur), _record(val), f"replay at word {word}")


@pytest.mark.parametrize("use_per", [True, False])
@pytest.mark.parametrize("word", [0, -3])
def test_a_bad_word_samples_as_from_one_row_and_raises_the_bit(dev, word, use_per):
    from prism_amd import _native as N
    val, cur = _twins(dev, use_per=use_per)
    buf = cur.experience_buffer
    before = _ring(cur)
    buf._cursor_words[0] = word
    buf._cursor_words[1] = CAP
    _front(val, size=1)
    _front(cur, slot=0)
    want, got = _record(val), _record(cur)
    try:
        assert int(got.pop("status").item()) == N.STATUS_FRONT_BAD_SIZE == 32 and int(want.pop("status").item()) == 0
        with pytest.raises(RuntimeError, match="prism_step_front_cursor"):
            buf.check_status()
    finally:
        buf.status.zero_()                                      # (sticky; the twins are shared)
    _same(got, want, f"word {word}")
    assert got["index"].tolist() == [0] * 16
    _same(_ring(cur), before, "the ring after the launch")
    assert buf._cursor_words.tolist() == [word, CAP]
