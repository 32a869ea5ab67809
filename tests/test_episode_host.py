"""No GPU needed: the episode bookkeeping's host side.  ``EpisodeHost`` (tests/episode_cases.py, the checker of the device)
against what the live reference's collector recorded in ``tests/golden/collector_bookkeeping.npz``, exactly; the argument
checks of ``prism_replay_ingest_tracked`` through the C ABI; how ``HipReplayBuffer`` reads ``reward_clipping_type``."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import episode_cases as EC
from tests import helpers as H


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from prism_amd import _native as N
    if not os.path.exists(N.LIB_PATH):
        g.build()
    return N.lib()


@pytest.fixture(scope="module")
def golden():
    return dict(np.load(EC.GOLDEN))


def _replay(g, tag, **kw):
    """The fixture's timesteps, in the order they reached the reference's buffer, through an EpisodeHost."""
    host = EC.EpisodeHost(ema=float(g["ema"]), **kw)
    S = int(g["n_streams"])
    raw = g["raw_reward"]
    out = []
    for k, e in enumerate(g[tag + "_stream"]):
        out.append(host.step(int(e), raw[e, k // S], g[tag + "_done"][k], g[tag + "_truncated"][k]))
    return host, out


@pytest.mark.parametrize("tag,clip", [("none", None), ("clamp", "dopamine_clamp")])
def test_episode_host_reproduces_the_reference_exactly(golden, tag, clip):
    """Three streams interleaved, 60 steps each: every stored reward bit for bit, every episodic return and every value of
    the training reward in float64 equality; None until the first episode has ended."""
    g = golden
    host, out = _replay(g, tag, clip=clip)
    assert len(out) == 180 and list(g[tag + "_stream"][:6]) == [0, 1, 2, 0, 1, 2]
    stored = np.array([o[0] for o in out], np.float32)
    np.testing.assert_array_equal(EC.bits32(stored), EC.bits32(g[tag + "_stored_reward"]))
    np.testing.assert_array_equal(EC.bits64([o[1] for o in out]), EC.bits64(g[tag + "_episodic_reward"]))
    valid = np.array([o[2] is not None for o in out])
    np.testing.assert_array_equal(valid, g[tag + "_training_valid"])
    got = np.array([o[2] for o in out if o[2] is not None], np.float64)
    np.testing.assert_array_equal(EC.bits64(got), EC.bits64(g[tag + "_training_reward"][valid]))
    # the fixture holds what the issue lists: a done on a first step, a truncation, both at once, one-step episodes,
    # rewards on both sides of +-1, and sums float32 could not hold
    ends = g[tag + "_done"] | g[tag + "_truncated"]
    assert g[tag + "_done"][0] and g[tag + "_episodic_reward"][0] == 0.0 and valid[0]
    assert (g[tag + "_done"] & g[tag + "_truncated"]).any() and (~g[tag + "_done"] & g[tag + "_truncated"]).any()
    assert host.stats()["episodes"] == int(ends.sum()) >= 10 and host.stats()["rows"] == 180
    ep = g[tag + "_episodic_reward"]
    assert (ep.astype(np.float32).astype(np.float64) != ep).any()
    if clip:
        raw = np.array([g["raw_reward"][e, k // 3] for k, e in enumerate(g[tag + "_stream"])])
        assert np.abs(stored).max() == 1.0 and (np.abs(raw) > 1).sum() > 20
        np.testing.assert_array_equal(EC.bits32(stored), EC.bits32(EC.clamp_f32(raw)))
        one = np.float32(1)
        for v in (np.nextafter(one, np.float32(0)), -np.nextafter(one, np.float32(0)), np.float32(0)):
            assert (stored == v).any()                      # kept: just inside the clamp, and zero


def test_clip_does_not_change_the_returns(golden):
    for k in ("episodic_reward", "training_reward", "training_valid"):
        np.testing.assert_array_equal(golden["none_" + k], golden["clamp_" + k])


def test_count_first_step_differs_by_each_episodes_first_reward(golden):
    """count_first_step=True: every timestep's episodic return is the fixture's plus the first reward of its episode -- and
    nothing else (checked in exact rational arithmetic on the rewards, then against the float64 sum step by step)."""
    g = golden
    _, ref = _replay(g, "none")
    _, got = _replay(g, "none", count_first_step=True)
    S = int(g["n_streams"])
    from fractions import Fraction
    first, prev, rounded, exact_rows = {}, {}, {}, 0
    for k, e in enumerate(g["none_stream"]):
        e = int(e)
        r = float(g["raw_reward"][e, k // S])
        if e not in first:
            first[e], want, rounded[e] = r, r, False         # the episode's first step: the fixture says 0, this says r
            assert ref[k][1] == 0.0
        else:
            want = r + prev[e]                               # same recurrence, started at the first reward instead of 0
        assert got[k][1] == want
        # the rewards are float32 values of magnitude >= 2^-10 (lowest bit 2^-33 or above): a float64 sum of them is exact
        # while it stays below 2^20, so until an episode's sums reach that the two differ by the first reward EXACTLY
        rounded[e] = rounded[e] or max(abs(got[k][1]), abs(ref[k][1])) >= 2.0 ** 20
        if not rounded[e]:
            assert Fraction(got[k][1]) - Fraction(ref[k][1]) == Fraction(first[e]), k
            exact_rows += 1
        prev[e] = got[k][1]
        if g["none_done"][k] or g["none_truncated"][k]:
            del first[e], prev[e]
    assert exact_rows > 40
    assert sum(a[1] != b[1] for a, b in zip(got, ref)) > 100


def _fake_ring(capacity=100, tree_capacity=128):
    from prism_amd import _native as N
    d = N.ReplayDesc()
    d.capacity, d.tree_capacity, d.obs_elems, d.n_step = capacity, tree_capacity, 400, 3
    addr = 0x10000000
    for f in ("obs", "succ_obs", "reward", "action", "flags", "link", "back", "tree", "per_state", "status"):
        setattr(d, f, addr)
        addr += 0x1000000
    return d


# (the one broken argument -- "ep__x": field x of the episode descriptor -- and text the message must carry)
TRACKED_REFUSALS = [
    (dict(ep=None), b"null episode descriptor"),
    (dict(ep__reward_clip=2), b"reward_clip must be PRISM_CLIP_NONE or PRISM_CLIP_CLAMP"),
    (dict(ep__reward_clip=-1), b"reward_clip must be PRISM_CLIP_NONE or PRISM_CLIP_CLAMP"),
    (dict(ep__ema=float("nan")), b"ema must be finite and in [0, 1]"),
    (dict(ep__ema=float("inf")), b"ema must be finite and in [0, 1]"),
    (dict(ep__ema=-0.01), b"ema must be finite and in [0, 1]"),
    (dict(ep__ema=1.5), b"ema must be finite and in [0, 1]"),
    (dict(ep__stats=None), b"must be all set or all NULL"),
    (dict(ep__ep_return=None, ep__ep_length=None, ep__stats=None), b"must be all set or all NULL"),
    (dict(ep__count_first_step=2), b"count_first_step must be 0 or 1"),
    (dict(ep__count_first_step=-1), b"count_first_step must be 0 or 1"),
    (dict(n=0), b"n must be in [1, capacity]"),                     # inherited from prism_replay_ingest
    (dict(rp=None), b"null descriptor"),
]


@pytest.mark.parametrize("case", range(len(TRACKED_REFUSALS)))
def test_tracked_argument_checks_without_device(lib, case):
    """Every refusal prism_replay_ingest_tracked adds to prism_replay_ingest's, and two it inherits: each case breaks ONE
    condition of a call every check accepts, over made-up addresses, so it returns before any HIP call."""
    from prism_amd import _native as N
    edit, text = TRACKED_REFUSALS[case]
    d = _fake_ring()
    a = 0x40000000
    ep = N.EpisodeDesc(reward_clip=N.CLIP_CLAMP, count_first_step=0, ema=0.9, ep_return=a, ep_length=a, stats=a, counts=a)
    kw = dict(rp=ctypes.byref(d), ep=ctypes.byref(ep), n=4)
    for k, v in edit.items():
        if k.startswith("ep__"):
            setattr(ep, k[4:], v)
        else:
            kw[k] = v
    rc = lib.prism_replay_ingest_tracked(kw["rp"], kw["n"], 7, 207, a, a, 0, a, a, a, a, None, a, 8, 0.5, 1e-8, kw["ep"], None)
    assert rc == N.PRISM_ERR_INVALID, (rc, lib.prism_last_error())
    assert text in lib.prism_last_error(), lib.prism_last_error()
    assert b"prism_replay_ingest_tracked" in lib.prism_last_error() or kw["rp"] is None


_C_TYPES = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "double": ctypes.c_double}


def test_episode_desc_matches_the_header_and_the_symbol_is_bound(lib):
    """The ctypes mirror against the struct as include/prism_hip.h declares it: field names, order, offsets and size."""
    from prism_amd import _native as N
    src = re.sub(r"/\*.*?\*/", "", open(N.HEADER_PATH).read(), flags=re.S)
    body = re.search(r"typedef struct prism_episode_desc \{(.*?)\} prism_episode_desc;", src, re.S).group(1)
    fields = []
    for decl in filter(None, (x.strip() for x in body.split(";"))):
        m = re.fullmatch(r"(\w+)\s*(\*?)\s*(\w+)", decl)
        fields.append((m.group(3), ctypes.c_void_p if m.group(2) else _C_TYPES[m.group(1)]))

    class FromHeader(ctypes.Structure):
        _fields_ = fields
    assert [f[0] for f in N.EpisodeDesc._fields_] == [f[0] for f in fields]
    assert ctypes.sizeof(N.EpisodeDesc) == ctypes.sizeof(FromHeader) == 48
    for name, _ in fields:
        assert getattr(N.EpisodeDesc, name).offset == getattr(FromHeader, name).offset, name
    assert re.search(r"#define PRISM_CLIP_NONE\s+0\b", src) and re.search(r"#define PRISM_CLIP_CLAMP\s+1\b", src)
    assert (N.CLIP_NONE, N.CLIP_CLAMP) == (0, 1)
    assert hasattr(ctypes.CDLL(N.LIB_PATH), "prism_replay_ingest_tracked")
    assert N.SIGNATURES["prism_replay_ingest_tracked"][1][-2:] == [ctypes.POINTER(N.EpisodeDesc), ctypes.c_void_p]
    assert N.SIGNATURES["prism_replay_ingest_tracked"][1][:-2] == N.SIGNATURES["prism_replay_ingest"][1][:-1]
    assert lib.prism_abi_version() == 3


def test_sign_raises_from_extend_batch_before_anything_is_allocated(lib):
    """``"sign"`` is the reference's r / abs(r): refused at the first extend_batch -- not at construction, where the
    reference's own collector (which clips before extend()) may still be the one that feeds the buffer."""
    from prism_amd.experience import HipReplayBuffer
    buf = HipReplayBuffer(16, 4, reward_clipping_type="sign")
    o, z = np.zeros((3, 7), np.float32), np.zeros(3, np.float32)
    with pytest.raises(ValueError, match="division by zero"):
        buf.extend_batch(o, o, z.astype(np.int32), z, z.astype(bool), z.astype(bool))
    assert buf._desc is None and buf._stream_tab is None and buf._ing is None and len(buf) == 0 and buf._serial == 0


@pytest.mark.parametrize("value,clamps", [("dopamine_clamp", True), ("dopamine_clip", False), ("none", False), (None, False),
                                          (("dopamine clamp",), False), ("sign", False), ("DOPAMINE_CLAMP", False)])
def test_only_dopamine_clamp_selects_the_clamp(lib, value, clamps):
    """Compared as the reference compares it: DEFAULT_CONFIG's "dopamine_clip" and the ablation presets' tuple clip nothing."""
    from prism_amd import _native as N
    from prism_amd.experience import HipReplayBuffer
    buf = HipReplayBuffer(16, 4, reward_clipping_type=value)
    assert buf._clip == (N.CLIP_CLAMP if clamps else N.CLIP_NONE)
    assert buf.reward_clipping_type == value and buf._ep is None


def test_factory_passes_the_configs_clipping_type(lib, monkeypatch):
    from prism_amd.config import baseline_config
    from prism_amd.factory import exp_buffer_factory
    seen = {}
    monkeypatch.setattr(exp_buffer_factory, "HipReplayBuffer", lambda **kw: seen.update(kw))
    for value in ("dopamine_clamp", ("dopamine clamp",)):
        exp_buffer_factory.build_exp_buffer(baseline_config(2, reward_clipping_type=value))
        assert seen["reward_clipping_type"] == value


def test_track_episodes_refuses_a_bad_ema_without_a_device(lib):
    from prism_amd.experience import HipReplayBuffer
    buf = HipReplayBuffer(16, 4)
    for ema in (-0.1, 1.1, float("nan")):
        with pytest.raises(ValueError, match="ema"):
            buf.track_episodes(ema)
    with pytest.raises(RuntimeError, match="track_episodes"):
        buf.episode_stats()
    assert buf._ep is None and buf._stream_tab is None


def test_untracked_kernel_keeps_its_name_and_both_have_no_private_segment(tmp_path):
    """Both kernels of the translation unit are there by name (the untracked launch is its own kernel, not a flag)."""
    import shutil
    import subprocess
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    csrc = os.path.join(H.ROOT, "prism_amd", "csrc")
    out = tmp_path / "ingest.s"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off",
                    "-I" + os.path.join(H.ROOT, "include"), "-I" + csrc, "-S", "--cuda-device-only", "-o", str(out),
                    os.path.join(csrc, "ingest.hip")], check=True, timeout=600, stdout=subprocess.DEVNULL,
                   stderr=subprocess.DEVNULL)
    kernels = dict(re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", out.read_text(), re.S))
    names = [k for k in kernels if "replay_ingest" in k]
    assert len(names) == 2 and sum("replay_ingest_tracked_kernel" in k for k in names) == 1
    for k in names:
        assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", kernels[k]).group(1)) == 0, k
