"""No GPU needed: the host side of ``prism_step_front_cursor`` (the fused step's front launch with the ring's size read from
device memory, for a launch a hipGraph replays while the ring fills) -- the symbol declared, exported and bound, every
host-side refusal through the C ABI, and the emitted gfx950 kernels' private segment."""
import ctypes
import os
import re
import shutil
import subprocess

import pytest

from tests import helpers as H

NAME = "prism_step_front_cursor"
_A = 0x40000000          # a made-up, 16-byte-aligned device address


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from prism_amd import _native as N
    if not os.path.exists(N.LIB_PATH):
        g.build()
    return N.lib()


def test_the_symbol_is_declared_exported_and_bound(lib):
    from prism_amd import _native as N
    header = open(os.path.join(H.ROOT, "include", "prism_hip.h")).read()
    assert re.search(r"^int\s+" + NAME + r"\s*\(", header, re.M), "not declared in include/prism_hip.h"
    assert hasattr(ctypes.CDLL(N.LIB_PATH), NAME)
    S = N.SIGNATURES
    assert NAME in S and len(S[NAME][1]) == 12
    # prism_step_front_ring's list with `size` replaced by the cursor words and the slot
    ring = S["prism_step_front_ring"][1]
    assert S[NAME][1] == ring[:3] + [N.c_vp, N.c_i32] + ring[4:]
    fn = getattr(lib, NAME)
    assert fn.argtypes == S[NAME][1] and fn.restype is ctypes.c_int
    assert lib.prism_abi_version() == 3          # the change is additive


def test_the_status_bit_is_a_power_of_two_of_its_own_and_mirrored():
    from prism_amd import _native as N
    header = open(os.path.join(H.ROOT, "include", "prism_hip.h")).read()
    bit = int(re.search(r"#define PRISM_STATUS_FRONT_BAD_SIZE (\d+)", header).group(1))
    others = [int(v) for v in re.findall(r"#define PRISM_STATUS_(?!FRONT_BAD_SIZE)\w+ (\d+)", header)]
    assert bit == N.STATUS_FRONT_BAD_SIZE == 32 and bit & (bit - 1) == 0 and bit not in others
    assert len(others) >= 5 and N.STATUS_INGEST_BAD_CURSOR in others


# (the one broken argument, the text the message must carry)
REFUSALS = [
    (dict(ring_kind=2), b"prism_step_front_cursor: ring_kind must be PRISM_RING_F32 or PRISM_RING_U8"),
    (dict(ring_kind=-1), b"prism_step_front_cursor: ring_kind must be PRISM_RING_F32 or PRISM_RING_U8"),
    (dict(ring_kind=1, rp=dict(obs=0x20000001)), b"prism_step_front_cursor: a byte ring's obs / succ_obs must be 4-byte aligned"),
    (dict(ring_kind=1, rp=dict(succ_obs=0x30000002)), b"prism_step_front_cursor: a byte ring's obs / succ_obs must be 4-byte aligned"),
    (dict(cursor=None), b"prism_step_front_cursor: null cursor"),
    (dict(slot=2), b"prism_step_front_cursor: slot must be 0 or 1"),
    (dict(slot=-1), b"prism_step_front_cursor: slot must be 0 or 1"),
    (dict(out_index=None), b"prism_step_front_cursor: null outputs"),
    (dict(out_weight=None, rp=dict(tree=0x50000000)), b"prism_step_front_cursor: null outputs"),   # PER needs the weights
    # the checks every front launch shares name the routine that holds them
    (dict(ld=None), b"check_learner: null descriptor"),
    (dict(rp=None), b"check_replay_for_step: null replay descriptor"),
    (dict(rp=dict(obs_elems=401)), b"check_replay_for_step: replay obs_elems must equal 10*10*C"),
    (dict(rp=dict(n_step=16)), b"check_replay_for_step: n_step out of range"),
    (dict(rp=dict(n_step=0)), b"check_replay_for_step: n_step out of range"),
    (dict(ring_kind=1, rp=dict(n_step=16)), b"check_replay_for_step: n_step out of range"),
]


@pytest.mark.parametrize("case", range(len(REFUSALS)))
def test_cursor_front_argument_checks_without_device(lib, case):
    from tests.test_abi import _fake_learner_desc
    edit, text = REFUSALS[case]
    ld, rp = _fake_learner_desc(lib, 2)
    rp.obs, rp.succ_obs = 0x20000000, 0x30000000
    kw = dict(ld=ctypes.byref(ld), rp=ctypes.byref(rp), ring_kind=0, cursor=0x60000000, slot=1, out_index=_A, out_weight=_A)
    for k, v in edit.items():
        if k == "rp" and isinstance(v, dict):
            for f, x in v.items():
                setattr(rp, f, x)
        else:
            kw[k] = v
    rc = getattr(lib, NAME)(kw["ld"], kw["rp"], kw["ring_kind"], kw["cursor"], kw["slot"], None, 1, 0, 0.4, kw["out_index"],
                            kw["out_weight"], None)
    assert rc == -1, (rc, lib.prism_last_error())
    assert text in lib.prism_last_error(), lib.prism_last_error()


@pytest.mark.parametrize("field,value,rc,text", [
    ("params", None, -1, b"check_learner: null parameter buffers"),
    ("out_td", None, -1, b"check_learner: null outputs"),
    ("obs", None, -1, b"check_learner: null batch arrays"),
    ("batch", 33, -3, b"not covered by the HIP kernels"),
])
def test_the_shared_learner_checks_still_fire(lib, field, value, rc, text):
    """check_learner's own conditions, through the new entry point (tests/test_abi.py holds the whole list to the by-value
    one)."""
    from tests.test_abi import _fake_learner_desc
    ld, rp = _fake_learner_desc(lib, 2)
    setattr(ld, field, value)
    got = getattr(lib, NAME)(ctypes.byref(ld), ctypes.byref(rp), 0, 0x60000000, 0, None, 1, 0, 0.4, _A, _A, None)
    assert got == rc and text in lib.prism_last_error(), (got, lib.prism_last_error())


def test_the_size_check_stays_with_the_by_value_entry_points(lib):
    from tests.test_abi import _fake_learner_desc
    ld, rp = _fake_learner_desc(lib, 2)
    for size in (0, rp.capacity + 1):
        rc = lib.prism_step_front_ring(ctypes.byref(ld), ctypes.byref(rp), 0, size, None, 1, 0, 0.4, _A, _A, None)
        assert rc == -1 and b"size must be in (0, capacity]" in lib.prism_last_error(), lib.prism_last_error()


def test_the_knob_and_the_counter_exist_and_default_to_off():
    import inspect
    from prism_amd import config as C
    from prism_amd.agents.hip_agent import HipAgent
    from prism_amd.learner import Learner
    assert Learner().graph_while_filling is False
    assert "graph_while_filling" in C.__doc__
    assert inspect.signature(HipAgent.step_fused).parameters["fill_graph"].default is False
    assert "cursor_slot" in inspect.signature(HipAgent._launch_fused).parameters


def test_cursor_front_kernels_have_no_private_segment(tmp_path):
    """The wrappers hand the body a copy of the by-value argument struct with the size replaced: it must stay in registers
    (tests/test_abi.py: a kernel-argument struct that lands in scratch costs microseconds per launch).  The two kernels are
    a translation unit of their own (front_cursor.hip), which must not define the learner's kernels a second time."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    csrc = os.path.join(H.ROOT, "prism_amd", "csrc")
    out = tmp_path / "front_cursor.s"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off",
                    "-I" + os.path.join(H.ROOT, "include"), "-I" + csrc, "-S", "--cuda-device-only", "-o", str(out),
                    os.path.join(csrc, "front_cursor.hip")], check=True, timeout=900, stdout=subprocess.DEVNULL,
                   stderr=subprocess.DEVNULL)
    text = out.read_text()
    kernels = dict(re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, re.S))
    new = [k for k in kernels if "step_front" in k]
    assert len(new) == 2 and all("cursor" in k for k in new) and sum("byte_ring" in k for k in new) == 1, new
    lds = set()
    for name in new:
        seg = re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", kernels[name])
        assert seg is not None and int(seg.group(1)) == 0, (name, seg and seg.group(1))
        lds.add(int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", kernels[name]).group(1)))
    assert len(lds) == 1, lds
    # the learner's own kernels (the non-template ones of the headers this unit includes) are not defined here again
    for name in ("step_front_kernel", "step_front_byte_ring_kernel", "iqn_embed_kernel", "dqn_loss_kernel", "dqn1_act_kernel",
                 "iqn_post_kernel"):
        assert not any(name in k for k in kernels), name
    assert "front_cursor.hip" in open(os.path.join(csrc, "Makefile")).read()
