"""No GPU needed: the host side of ``prism_replay_ingest_cursor`` (the ring cursor read from device memory, for a launch a
hipGraph replays) -- the symbol declared, exported and bound, every host-side refusal through the C ABI, and the emitted
gfx950 kernels' private segment."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest
import torch

from tests import helpers as H

NAME = "prism_replay_ingest_cursor"


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from prism_amd import _native as N
    if not os.path.exists(N.LIB_PATH):
        g.build()
    return N.lib()


def _fake_ring(capacity=100, tree_capacity=128):
    """A descriptor every ring check accepts, over made-up 16-byte-aligned addresses (tests/test_ingest_host.py): each case
    below breaks ONE condition, so the call is refused before anything touches a device."""
    from prism_amd import _native as N
    d = N.ReplayDesc()
    d.capacity, d.tree_capacity, d.obs_elems, d.n_step = capacity, tree_capacity, 400, 3
    addr = 0x10000000
    for f in ("obs", "succ_obs", "reward", "action", "flags", "link", "back", "tree", "per_state", "status"):
        setattr(d, f, addr)
        addr += 0x1000000
    return d


def _episodes(**edit):
    from prism_amd import _native as N
    e = N.EpisodeDesc()
    e.reward_clip, e.count_first_step, e.ema = N.CLIP_NONE, 0, 0.9
    e.ep_return = e.ep_length = e.stats = e.counts = 0x50000000
    for k, v in edit.items():
        setattr(e, k, v)
    return e


def test_the_symbol_is_declared_exported_and_bound(lib):
    from prism_amd import _native as N
    header = open(os.path.join(H.ROOT, "include", "prism_hip.h")).read()
    assert re.search(r"^int\s+" + NAME + r"\s*\(", header, re.M), "not declared in include/prism_hip.h"
    assert NAME in N.SIGNATURES and len(N.SIGNATURES[NAME][1]) == 19
    fn = getattr(lib, NAME)
    assert fn.argtypes == N.SIGNATURES[NAME][1] and fn.restype is ctypes.c_int
    assert lib.prism_abi_version() == 3          # the change is additive
    bit = int(re.search(r"#define PRISM_STATUS_INGEST_BAD_CURSOR (\d+)", header).group(1))
    others = [int(v) for v in re.findall(r"#define PRISM_STATUS_(?!INGEST_BAD_CURSOR)\w+ (\d+)", header)]
    assert bit == N.STATUS_INGEST_BAD_CURSOR and bit & (bit - 1) == 0 and bit not in others


# (the one broken argument, text the message must carry)
REFUSALS = [
    (dict(rp=None), b"null descriptor"),
    (dict(cursor=None), b"null cursor"),
    (dict(slot=2), b"slot must be 0 or 1"),
    (dict(slot=-1), b"slot must be 0 or 1"),
    (dict(n=0), b"n must be in [1, capacity]"),
    (dict(n=101), b"n must be in [1, capacity]"),
    (dict(n_streams=0), b"n_streams must be in [1, 65536]"),
    (dict(n_streams=65537), b"n_streams must be in [1, 65536]"),
    (dict(obs_kind=2), b"obs_kind"),
    (dict(obs_kind=-1), b"obs_kind"),
    (dict(ring_kind=2), b"ring_kind"),
    (dict(ring_kind=-1), b"ring_kind"),
    (dict(stream_tab=None), b"stream_tab"),
    (dict(obs=None), b"null transition array"),
    (dict(next_obs=None), b"null transition array"),
    (dict(reward=None), b"null transition array"),
    (dict(action=None), b"null transition array"),
    (dict(done=None), b"null transition array"),
    (dict(truncated=None), b"null transition array"),
    (dict(n=9, n_streams=8), b"stream_ids"),              # identity ids: row 8 would be stream 8 of 8
    (dict(ep=dict(stats=None)), b"all set or all NULL"),      # a partly filled episode descriptor
    (dict(ep=dict(ep_return=None, ep_length=None)), b"all set or all NULL"),
    (dict(ep=dict(reward_clip=7)), b"reward_clip"),
    (dict(ep=dict(ema=1.5)), b"ema"),
    (dict(ep=dict(count_first_step=2)), b"count_first_step"),
]


@pytest.mark.parametrize("case", range(len(REFUSALS)))
def test_cursor_ingest_argument_checks_without_device(lib, case):
    edit, text = REFUSALS[case]
    d = _fake_ring()
    a = 0x40000000
    kw = dict(rp=ctypes.byref(d), ring_kind=0, n=4, cursor=0x60000000, slot=1, obs=a, next_obs=a, obs_kind=0, reward=a,
              action=a, done=a, truncated=a, stream_ids=None, stream_tab=a, n_streams=8, ep=None)
    kw.update(edit)
    ep = None if kw["ep"] is None else ctypes.byref(_episodes(**kw["ep"]))
    rc = getattr(lib, NAME)(kw["rp"], kw["ring_kind"], kw["n"], kw["cursor"], kw["slot"], kw["obs"], kw["next_obs"],
                            kw["obs_kind"], kw["reward"], kw["action"], kw["done"], kw["truncated"], kw["stream_ids"],
                            kw["stream_tab"], kw["n_streams"], 0.5, 1e-8, ep, None)
    assert rc == -1, (rc, lib.prism_last_error())
    assert text in lib.prism_last_error(), lib.prism_last_error()
    # the message names the entry point that was called (the ring's own checks name the routine all entry points share)
    assert NAME.encode() in lib.prism_last_error() or lib.prism_last_error().startswith(b"check_ring")


@pytest.mark.parametrize("n_step", [0, 16])
def test_cursor_ingest_shares_the_ring_check(lib, n_step):
    d = _fake_ring()
    d.n_step = n_step
    a = 0x40000000
    rc = getattr(lib, NAME)(ctypes.byref(d), 0, 4, 0x60000000, 0, a, a, 0, a, a, a, a, None, a, 8, 0.5, 1e-8, None, None)
    assert rc == -1 and b"n_step out of range" in lib.prism_last_error(), lib.prism_last_error()


def test_cursor_methods_refuse_before_any_launch(lib):
    """The buffer's enqueue-only call needs everything in place beforehand: nothing is allocated on its behalf."""
    from prism_amd.experience import HipReplayBuffer
    buf = HipReplayBuffer(16, 4)
    with pytest.raises(RuntimeError, match="must exist before"):
        buf.enqueue_extend_cursor(0, torch.zeros(3, 7), None, None, None, None, None)
    assert buf._desc is None and buf._serial == 0 and buf._cursor_known is None


def test_cursor_ingest_kernels_have_no_private_segment(tmp_path):
    """The wrappers hand the body a copy of the by-value argument struct with the cursor's two words replaced: it must stay
    in registers (tests/test_abi.py: a kernel-argument struct that lands in scratch costs microseconds per launch)."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    csrc = os.path.join(H.ROOT, "prism_amd", "csrc")
    out = tmp_path / "ingest.s"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off",
                    "-I" + os.path.join(H.ROOT, "include"), "-I" + csrc, "-S", "--cuda-device-only", "-o", str(out),
                    os.path.join(csrc, "ingest.hip")], check=True, timeout=600, stdout=subprocess.DEVNULL,
                   stderr=subprocess.DEVNULL)
    text = out.read_text()
    kernels = dict(re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, re.S))
    new = [k for k in kernels if "cursor_ingest" in k]
    assert len(new) == 4 and sum("tracked" in k for k in new) == 2 and sum("byte_ring" in k for k in new) == 2, new
    for name in new:
        seg = re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", kernels[name])
        assert seg is not None and int(seg.group(1)) == 0, (name, seg and seg.group(1))
    assert "scratch_" not in text
