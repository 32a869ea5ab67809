"""No GPU needed: the byte observation ring's host side (``HipReplayBuffer(obs_storage="uint8")``, ``PRISM_RING_U8``).

  1. the narrowing function of ``prism_amd/csrc/common.h`` -- the very text the kernels compile, built for the host alone --
     against its NumPy restatement (tests/obs_ring_cases.py ``narrow``): stored byte and exact flag;
  2. the argument checks of the four ``prism_*_ring`` entry points through the C ABI, old and new symbols side by side,
     struct sizes and ABI version unchanged;
  3. the knob ``config.replay_obs_storage`` and what the buffer refuses without touching a device;
  4. the fused-step cases of tests/test_gpu_obs_ring.py reach every successor class of the front launch."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import helpers as H
from tests import obs_ring_cases as OC


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from prism_amd import _native as N
    if not os.path.exists(N.LIB_PATH):
        g.build()
    return N.lib()


# ---------------------------------------------------------------------------------------------- 1. narrowing
_HOST_PROGRAM = r"""
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "common.h"
// in: n float bit patterns (n % 4 == 0); out: per value {byte, exact}, then per group of four {word of obs_narrow4 (4 bytes),
// any inexact, the four floats of obs_widen4 of that word}
int main(int argc, char **argv) {
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "wb");
    if (!in || !out) return 2;
    const long n = atol(argv[3]);
    uint32_t *bits = (uint32_t *)malloc(4 * n);
    if (fread(bits, 4, n, in) != (size_t)n) return 3;
    for (long i = 0; i < n; ++i) {
        float x;
        memcpy(&x, &bits[i], 4);
        bool inexact = false;
        const uint8_t rec[2] = {(uint8_t)prism::obs_narrow(x, inexact), (uint8_t)!inexact};
        fwrite(rec, 1, 2, out);
    }
    for (long i = 0; i < n; i += 4) {
        float4 v;
        memcpy(&v, &bits[i], 16);
        bool inexact = false;
        const uint32_t w = prism::obs_narrow4(v, inexact);
        const uint32_t flag = inexact;
        const float4 back = prism::obs_widen4(w);
        fwrite(&w, 4, 1, out);
        fwrite(&flag, 4, 1, out);
        fwrite(&back, 16, 1, out);
    }
    fclose(out);
    return 0;
}
"""


def _hipcc():
    cand = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    return cand if os.path.isfile(cand) and os.access(cand, os.X_OK) else None


def test_common_h_narrowing_on_the_host_equals_the_numpy_restatement(tmp_path):
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("no hipcc to compile the host program with")
    src, exe = tmp_path / "narrow_host.cpp", tmp_path / "narrow_host"
    src.write_text(_HOST_PROGRAM)
    subprocess.run([hipcc, "-x", "hip", "--offload-host-only", "-O1", "-std=c++17", "-ffp-contract=off",
                    "-I", os.path.join(H.ROOT, "include"), "-I", os.path.join(H.ROOT, "prism_amd", "csrc"),
                    str(src), "-o", str(exe)], check=True, capture_output=True, text=True, timeout=300)
    named = np.array([-0.0, np.nan, np.inf, -np.inf, 0.5, -1.0, 255.5, 256.0], np.float32)
    rng = np.random.default_rng(20)
    byte_bits = np.arange(256, dtype=np.float32).view(np.uint32)
    x = np.concatenate([np.arange(256, dtype=np.float32), named,
                        rng.integers(0, 2 ** 32, 100_000, dtype=np.uint64).astype(np.uint32).view(np.float32),
                        (byte_bits + np.uint32(1)).view(np.float32), (byte_bits - np.uint32(1)).view(np.float32)])
    assert x.size % 4 == 0
    (tmp_path / "in.bin").write_bytes(x.tobytes())
    subprocess.run([str(exe), str(tmp_path / "in.bin"), str(tmp_path / "out.bin"), str(x.size)], check=True, timeout=60)
    raw = (tmp_path / "out.bin").read_bytes()
    rec = np.frombuffer(raw[:2 * x.size], np.uint8).reshape(-1, 2)
    want_b, want_exact = OC.narrow(x)
    np.testing.assert_array_equal(rec[:, 0], want_b)
    np.testing.assert_array_equal(rec[:, 1].astype(bool), want_exact)
    # the rule itself, on the named values: every byte is itself and exact, none of the others is, all of them store 0
    np.testing.assert_array_equal(want_b[:256], np.arange(256))
    assert want_exact[:256].all() and not want_exact[256:264].any() and not want_b[256:264].any()
    assert want_exact[264:100_264].sum() < 100                   # (random patterns: next to none is byte-exact)
    assert not want_exact[100_264:].any()                        # (one unit in the last place beside a byte, either side)
    groups = np.frombuffer(raw[2 * x.size:], np.uint32).reshape(-1, 6)
    np.testing.assert_array_equal(groups[:, 0].copy().view(np.uint8).reshape(-1, 4), want_b.reshape(-1, 4))
    np.testing.assert_array_equal(groups[:, 1].astype(bool), ~want_exact.reshape(-1, 4).all(axis=1))
    np.testing.assert_array_equal(groups[:, 2:].copy().view(np.float32).view(np.uint32),
                                  want_b.reshape(-1, 4).astype(np.float32).view(np.uint32))


# ---------------------------------------------------------------------------------------------- 2. C ABI
def _fake_ring(capacity=100, tree_capacity=128, obs_elems=400):
    from prism_amd import _native as N
    d = N.ReplayDesc()
    d.capacity, d.tree_capacity, d.obs_elems, d.n_step = capacity, tree_capacity, obs_elems, 3
    addr = 0x10000000
    for f in ("obs", "succ_obs", "reward", "action", "flags", "link", "back", "tree", "per_state", "status"):
        setattr(d, f, addr)
        addr += 0x1000000
    return d


_A = 0x40000000
ENTRY = {
    "insert": lambda lib, rp, kind, kw: lib.prism_replay_insert_ring(rp, kind, kw.get("n", 4), _A, kw.get("obs", _A), _A,
                                                                     kw.get("obs_kind", 1), _A, _A, _A, _A, 0.5, 1e-8, None),
    "ingest": lambda lib, rp, kind, kw: lib.prism_replay_ingest_ring(rp, kind, kw.get("n", 4), 7, 207, kw.get("obs", _A), _A,
                                                                     kw.get("obs_kind", 1), _A, _A, _A, _A, None, _A, 8, 0.5,
                                                                     1e-8, kw.get("ep"), None),
    "gather": lambda lib, rp, kind, kw: lib.prism_replay_gather_ring(rp, kind, _A, kw.get("n", 4), kw.get("obs", _A), _A, _A, _A,
                                                                     _A, _A, None),
}
# (entry point, ring kind, edit of the descriptor, other arguments, text): every call fails a check before any HIP call
RING_REFUSALS = [(e, kind, None, {}, b"prism_replay_%s_ring: ring_kind must be PRISM_RING_F32 or PRISM_RING_U8" % e.encode())
                 for e in ENTRY for kind in (2, -1)]
RING_REFUSALS += [(e, 1, "null", {}, b"null descriptor") for e in ENTRY]
RING_REFUSALS += [(e, 1, dict(n_step=16), {}, b"n_step out of range") for e in ENTRY]
RING_REFUSALS += [(e, 1, dict(tree_capacity=64), {}, b"tree_capacity") for e in ENTRY]
RING_REFUSALS += [(e, 1, dict(succ_obs=None), {}, b"null ring array") for e in ENTRY]
RING_REFUSALS += [(e, 1, dict(obs=0x10000002), {}, b"a byte ring's obs / succ_obs must be 4-byte aligned") for e in ENTRY]
RING_REFUSALS += [
    ("insert", 1, None, dict(n=101), b"n must be in (0, capacity]"),
    ("insert", 1, None, dict(obs=None), b"null staging array"),
    ("insert", 0, None, dict(obs_kind=2), b"prism_replay_insert_ring: obs_kind"),
    ("insert", 0, None, dict(obs_kind=1), b"prism_replay_insert_ring: an fp32 ring takes fp32 staging rows"),
    ("ingest", 1, None, dict(n=0), b"n must be in [1, capacity]"),
    ("ingest", 1, None, dict(obs_kind=2), b"obs_kind"),
    ("ingest", 1, None, dict(obs=None), b"null transition array"),
    ("ingest", 1, None, dict(ep="bad clip"), b"reward_clip"),
    ("ingest", 0, None, dict(ep="bad ema"), b"ema must be finite"),
    ("gather", 1, None, dict(n=0), b"batch/out"),
    ("gather", 0, None, dict(obs=None), b"batch/out"),
]


@pytest.mark.parametrize("case", range(len(RING_REFUSALS)))
def test_ring_entry_points_check_their_arguments_without_a_device(lib, case):
    from prism_amd import _native as N
    entry, kind, edit, kw, text = RING_REFUSALS[case]
    d = _fake_ring()
    if isinstance(edit, dict):
        for k, v in edit.items():
            setattr(d, k, v)
    kw = dict(kw)
    if isinstance(kw.get("ep"), str):
        ep = N.EpisodeDesc()
        ep.ema = 0.9
        if kw["ep"] == "bad clip":
            ep.reward_clip = 7
        else:
            ep.ema = float("nan")
        kw["ep"] = ctypes.byref(ep)
    rc = ENTRY[entry](lib, None if edit == "null" else ctypes.byref(d), kind, kw)
    assert rc == -1, (rc, lib.prism_last_error())
    assert text in lib.prism_last_error(), lib.prism_last_error()


def _fake_learner(lib):
    from tests.test_abi import _fake_learner_desc
    return _fake_learner_desc(lib, 2)


@pytest.mark.parametrize("kind,edit,text", [
    (2, None, b"prism_step_front_ring: ring_kind must be PRISM_RING_F32 or PRISM_RING_U8"),
    (-1, None, b"prism_step_front_ring: ring_kind must be PRISM_RING_F32 or PRISM_RING_U8"),
    (1, "null ld", b"check_learner: null descriptor"),
    (1, "null rp", b"check_replay_for_step: null replay descriptor"),
    (1, dict(obs_elems=401), b"check_replay_for_step: replay obs_elems must equal 10*10*C"),
    (0, dict(n_step=16), b"check_replay_for_step: n_step out of range"),
    (1, dict(obs=0x10000001), b"prism_step_front_ring: a byte ring's obs / succ_obs must be 4-byte aligned"),
    (1, "size", b"size must be in (0, capacity]"),
])
def test_front_ring_checks_its_arguments_without_a_device(lib, kind, edit, text):
    ld, rp = _fake_learner(lib)
    rp.obs, rp.succ_obs = 0x20000000, 0x30000000
    if isinstance(edit, dict):
        for k, v in edit.items():
            setattr(rp, k, v)
    p_ld = None if edit == "null ld" else ctypes.byref(ld)
    p_rp = None if edit == "null rp" else ctypes.byref(rp)
    rc = lib.prism_step_front_ring(p_ld, p_rp, kind, 0 if edit == "size" else 100, None, 1, 0, 0.4, _A, _A, None)
    assert rc == -1, (rc, lib.prism_last_error())
    assert text in lib.prism_last_error(), lib.prism_last_error()


def test_old_and_new_symbols_are_exported_and_the_structs_keep_their_sizes(lib):
    import re
    from prism_amd import _native as N
    raw = ctypes.CDLL(N.LIB_PATH)
    for old in ("prism_replay_insert", "prism_replay_ingest", "prism_replay_ingest_tracked", "prism_replay_gather",
                "prism_step_front"):
        assert hasattr(raw, old), old
    for new in ("prism_replay_insert_ring", "prism_replay_ingest_ring", "prism_replay_gather_ring", "prism_step_front_ring"):
        assert hasattr(raw, new) and new in N.SIGNATURES, new
    # the storage kind travels as an argument: right behind the descriptor(s), the rest as the old entry point has it
    S = N.SIGNATURES
    assert S["prism_replay_gather_ring"][1] == S["prism_replay_gather"][1][:1] + [N.c_i32] + S["prism_replay_gather"][1][1:]
    assert S["prism_step_front_ring"][1] == S["prism_step_front"][1][:2] + [N.c_i32] + S["prism_step_front"][1][2:]
    assert S["prism_replay_ingest_ring"][1] == S["prism_replay_ingest_tracked"][1][:1] + [N.c_i32] + \
        S["prism_replay_ingest_tracked"][1][1:]
    assert S["prism_replay_insert_ring"][1][:2] == [ctypes.POINTER(N.ReplayDesc), N.c_i32]
    assert ctypes.sizeof(N.ReplayDesc) == 8 + 8 + 4 + 4 + 10 * 8 + 16 * 8
    assert ctypes.sizeof(N.LearnerDesc) == 88 + 184 + 8 + 6 * 8 + 7 * 8 + 4 * 8 + 24 + 24 + 8 + 8 + 7 * 8 + 8 + 40 + 8
    assert lib.prism_abi_version() == 3
    src = open(N.HEADER_PATH).read()
    for name, value in (("PRISM_RING_F32", 0), ("PRISM_RING_U8", 1), ("PRISM_STATUS_OBS_INEXACT", 8)):
        assert re.search(r"#define %s\s+%d\b" % (name, value), src), name
    assert (N.RING_F32, N.RING_U8, N.STATUS_OBS_INEXACT) == (0, 1, 8)


# ---------------------------------------------------------------------------------------------- 3. the knob
def test_knob_default_uint8_and_unknown_values(lib, monkeypatch):
    from prism_amd import _native as N
    from prism_amd.config import baseline_config
    from prism_amd.experience import HipReplayBuffer
    from prism_amd.factory import exp_buffer_factory
    seen = {}
    monkeypatch.setattr(exp_buffer_factory, "HipReplayBuffer", lambda **kw: seen.update(kw))
    cfg = baseline_config(2)
    assert not hasattr(cfg, "replay_obs_storage")                # (not a dataclass field: old presets construct unchanged)
    exp_buffer_factory.build_exp_buffer(cfg)
    assert seen["obs_storage"] == "float32"
    cfg.replay_obs_storage = "uint8"
    exp_buffer_factory.build_exp_buffer(cfg)
    assert seen["obs_storage"] == "uint8"
    monkeypatch.undo()
    buf = exp_buffer_factory.build_exp_buffer(cfg)
    assert buf.obs_storage == "uint8" and buf._ring_kind == N.RING_U8 and buf._desc is None
    plain = HipReplayBuffer(16, 4)
    assert plain.obs_storage == "float32" and plain._ring_kind == N.RING_F32
    for bad in ("int8", "float16", None, 1):
        # (before the device argument is even looked at: a CPU device would be a NativeLibraryError)
        with pytest.raises(ValueError, match="obs_storage"):
            HipReplayBuffer(16, 4, device="cpu", obs_storage=bad)
    cfg.replay_obs_storage = "bytes"
    with pytest.raises(ValueError, match="obs_storage"):
        exp_buffer_factory.build_exp_buffer(cfg)


@pytest.mark.parametrize("bad", OC.INEXACT)
def test_host_side_inexact_observations_are_refused_before_anything_is_allocated(lib, bad):
    from prism_amd.experience import HipReplayBuffer, Timestep
    buf = HipReplayBuffer(16, 4, obs_storage="uint8")
    o = np.ones((3, 6), np.float32)
    spoiled = o.copy()
    spoiled[1, 4] = bad
    z = np.zeros(3, np.float32)
    for pair in ((spoiled, o), (o, spoiled)):
        with pytest.raises(ValueError, match="byte-exact"):
            buf.extend_batch(pair[0], pair[1], z.astype(np.int32), z, z.astype(bool), z.astype(bool))
    t, nxt = Timestep(id=0, obs=o[0]), Timestep(id=1, obs=spoiled[1])
    t.action, t.reward, t.done, t.truncated, t.next = 0, 0.0, False, False, nxt
    with pytest.raises(ValueError, match="byte-exact"):
        buf.extend(t)
    with pytest.raises(ValueError, match="byte-exact"):
        buf.extend(nxt)
    assert buf._desc is None and len(buf) == 0 and buf._serial == 0 and buf._n_staged == 0 and buf._ing is None
    assert buf.buffer._writer._cursor == 0


# ---------------------------------------------------------------------------------------------- 4. the case generator
def _buffer_seed():
    from prism_amd.config import baseline_config
    return baseline_config(2).seed


@pytest.mark.parametrize("name", list(OC.FUSED_CASES))
def test_fused_cases_sample_every_successor_class(name):
    """The slots a case's fused steps sample, as far as they follow from the ring alone (``known_indices``: all ten steps of
    uniform replay, the first step of prioritized replay), include the three successor classes.  A prioritized batch of two
    cannot hold three: its first step draws the two rare classes -- no successor, successor elsewhere -- and the GPU test
    requires the third among the slots of its ten steps."""
    case = OC.FUSED_CASES[name]
    orc, prio, obs_b, succ_b = OC.fused_ring(case)
    assert orc.capacity == 64 and orc.length == (64 if case.full else 40) and orc.n_step == 3
    idx = OC.known_indices(case, _buffer_seed())
    assert idx.size == (case.B if case.use_per else 10 * case.B)
    kinds = {OC.successor_class(orc, int(i)) for i in idx}
    want = {OC.NONE, OC.ELSEWHERE} if case.use_per and case.B == 2 else {OC.PRED, OC.NONE, OC.ELSEWHERE}
    assert kinds >= want, (name, kinds)
    # the bytes are the oracle's planes scaled: zero where they are zero, 255 somewhere, a linked successor still the row
    assert ((obs_b != 0) == (orc.obs != 0)).all() and obs_b.max() == 255 and {0, 1} < set(np.unique(obs_b).tolist())
    linked = np.flatnonzero(orc.link[:orc.length] >= 0)
    np.testing.assert_array_equal(succ_b[linked], obs_b[orc.link[linked]])


def test_fused_cases_cover_the_shapes_batches_and_both_samplers():
    cs = list(OC.FUSED_CASES.values())
    assert {(c.C, c.B) for c in cs if c.use_per and not c.full} == {(C, B) for C in (1, 4, 10) for B in (2, 16)}
    assert any(not c.use_per and not c.full for c in cs) and any(not c.use_per and c.full for c in cs)
    assert any(c.use_per and c.full for c in cs)
    assert [int(np.prod(s)) % 4 for s in OC.SHAPES] == [0, 0, 0, 2] and int(np.prod(OC.SHAPES[2])) // 4 == 250


def test_streams_feed_named_bytes_episode_ends_and_truncations():
    gen = OC.Streams((10, 10, 4), 8, seed=3)
    steps = [gen.step() for _ in range(14)]                      # 112 rows: three times round a ring of 37
    done = np.concatenate([s["done"] for s in steps])
    trunc = np.concatenate([s["truncated"] for s in steps])
    assert done.any() and trunc.any() and not (done & trunc).any() and (~done & ~trunc).sum() > 60
    for a, b in zip(steps, steps[1:]):                           # a stream goes on with its next observation
        go = ~(a["done"] | a["truncated"])
        np.testing.assert_array_equal(b["obs"][go], a["next_obs"][go])
    vals = np.unique(np.concatenate([s["obs"].ravel() for s in steps]))
    assert {0, 1, 255} <= set(vals.tolist()) and len(vals) > 5
    obs, succ, cursor = OC.expected_ring(37, steps)
    assert cursor == 112 % 37 and obs.any(axis=1).all()
    last_round = np.concatenate([np.stack([s["done"], s["truncated"]], 1) for s in steps])[112 - 37:]
    zero_rows = (~succ.any(axis=1)).sum()
    assert zero_rows == int((last_round[:, 0] & ~last_round[:, 1]).sum()) > 0
