"""No GPU needed: the vectorised producer seam's host side -- argument checks of ``prism_replay_ingest`` through the C ABI,
the emitted gfx950 kernel's private segment, and the stream table's serial rule against a host that tracks every slot."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import helpers as H


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from prism_amd import _native as N
    if not os.path.exists(N.LIB_PATH):
        g.build()
    return N.lib()


def _fake_ring(capacity=100, tree_capacity=128):
    """A descriptor every ring check accepts, over made-up 16-byte-aligned addresses: each case below breaks ONE condition,
    so the call is refused before anything touches a device."""
    from prism_amd import _native as N
    d = N.ReplayDesc()
    d.capacity, d.tree_capacity, d.obs_elems, d.n_step = capacity, tree_capacity, 400, 3
    addr = 0x10000000
    for f in ("obs", "succ_obs", "reward", "action", "flags", "link", "back", "tree", "per_state", "status"):
        setattr(d, f, addr)
        addr += 0x1000000
    return d


# (the one broken argument, text the message must carry)
INGEST_REFUSALS = [
    (dict(rp=None), b"null descriptor"),
    (dict(n=0), b"n must be in [1, capacity]"),
    (dict(n=101), b"n must be in [1, capacity]"),
    (dict(n_streams=0), b"n_streams must be in [1, 65536]"),
    (dict(n_streams=65537), b"n_streams must be in [1, 65536]"),
    (dict(obs_kind=2), b"obs_kind"),
    (dict(obs_kind=-1), b"obs_kind"),
    (dict(first_slot=100, serial0=100), b"first_slot"),
    (dict(first_slot=3, serial0=4), b"serial0"),
    (dict(stream_tab=None), b"stream_tab"),
    (dict(obs=None), b"null transition array"),
    (dict(n=9, n_streams=8), b"stream_ids"),              # identity ids: row 8 would be stream 8 of 8
]


@pytest.mark.parametrize("case", range(len(INGEST_REFUSALS)))
def test_ingest_argument_checks_without_device(lib, case):
    edit, text = INGEST_REFUSALS[case]
    d = _fake_ring()
    a = 0x40000000
    kw = dict(rp=ctypes.byref(d), n=4, first_slot=7, serial0=207, obs=a, next_obs=a, obs_kind=0, reward=a, action=a,
              done=a, truncated=a, stream_ids=None, stream_tab=a, n_streams=8)
    kw.update(edit)
    rc = lib.prism_replay_ingest(kw["rp"], kw["n"], kw["first_slot"], kw["serial0"], kw["obs"], kw["next_obs"],
                                 kw["obs_kind"], kw["reward"], kw["action"], kw["done"], kw["truncated"], kw["stream_ids"],
                                 kw["stream_tab"], kw["n_streams"], 0.5, 1e-8, None)
    assert rc == -1, (rc, lib.prism_last_error())
    assert text in lib.prism_last_error(), lib.prism_last_error()


@pytest.mark.parametrize("n_step", [0, 16])
def test_ingest_shares_the_ring_check_n_step_range(lib, n_step):
    """prism_replay_ingest runs the ring check every replay entry point runs: a descriptor whose n_step lies outside
    [1, PRISM_MAX_NSTEP = 15] is refused before any device is touched."""
    d = _fake_ring()
    d.n_step = n_step
    a = 0x40000000
    rc = lib.prism_replay_ingest(ctypes.byref(d), 4, 7, 207, a, a, 0, a, a, a, a, None, a, 8, 0.5, 1e-8, None)
    assert rc == -1, (rc, lib.prism_last_error())
    assert b"n_step out of range" in lib.prism_last_error(), lib.prism_last_error()


def test_extend_batch_rejects_host_side_ids_before_any_launch(lib):
    """Duplicate / out-of-range / miscounted ids in a HOST array are refused before the buffer allocates anything."""
    from prism_amd.experience import HipReplayBuffer
    buf = HipReplayBuffer(16, 4)
    o = np.zeros((3, 7), np.float32)
    z = np.zeros(3, np.float32)
    for ids, text in (([0, 1, 1], "distinct"), ([0, 1, 65536], "stream_ids must lie in"), ([-1, 0, 1], "stream_ids must lie in"),
                      ([0, 1], "one id per row")):
        with pytest.raises(ValueError, match=text):
            buf.extend_batch(o, o, z.astype(np.int32), z, z.astype(bool), z.astype(bool), stream_ids=np.array(ids))
    with pytest.raises(ValueError, match="next_obs"):
        buf.extend_batch(o.astype(np.uint8), o, z.astype(np.int32), z, z.astype(bool), z.astype(bool))
    with pytest.raises(ValueError, match="reserve_streams"):
        buf.reserve_streams(65537)
    with pytest.raises(ValueError, match="n = 17 rows"):
        buf.extend_batch(np.zeros((17, 7), np.float32), None, None, None, None, None)
    assert buf._desc is None and len(buf) == 0 and buf._serial == 0


def test_ingest_kernel_has_no_private_segment(tmp_path):
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
    kernels = re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, re.S)
    assert any("replay_ingest_kernel" in name for name, _ in kernels)
    for name, body in kernels:
        seg = re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", body)
        assert seg is not None and int(seg.group(1)) == 0, (name, seg and seg.group(1))


@pytest.mark.parametrize("capacity,n_streams,seed", [(7, 5, 0), (16, 4, 1), (37, 9, 2), (64, 3, 3)])
def test_serial_rule_equals_a_host_that_tracks_every_slot(capacity, n_streams, seed):
    """The kernel's rule -- stream table entry w = write serial of the stream's open row; predecessor valid iff
    serial - w < capacity, at slot w % capacity -- against the bookkeeping extend() does (an owner per slot, a pending
    (slot, row) per stream), over random interleavings with episode ends, truncations and absences of a stream longer than
    the ring.  Both drive a ReplayOracle row by row; predecessors and the oracles' links must agree at every row."""
    from oracle import per_ref
    rng = np.random.default_rng(seed)
    by_rule = per_ref.ReplayOracle(capacity, 1, 3, 0.99, use_per=False)
    by_host = per_ref.ReplayOracle(capacity, 1, 3, 0.99, use_per=False)
    tab = np.full(n_streams, -1, np.int64)                   # the rule's whole state (+ the serial)
    owner = np.full(capacity, -1, np.int64)                  # the host's: row id stored in every slot ...
    pending = {}                                             # ... and (slot, row id) of every stream's open row
    asleep = np.zeros(n_streams, np.int64)
    serial, linked, expired = 0, 0, 0
    for _ in range(60 * capacity):
        e = int(rng.integers(n_streams))
        if asleep[e] > 0:                                    # a long absence: the stream skips its turns
            asleep[e] -= 1
            continue
        if rng.random() < 0.02:
            asleep[e] = int(rng.integers(capacity // 2, 3 * capacity))
        done = bool(rng.random() < 0.07)
        trunc = bool(rng.random() < 0.03)
        # the rule
        w = tab[e]
        p_rule = int(w % capacity) if w >= 0 and serial - w < capacity else -1
        # the host
        slot = serial % capacity
        owner[slot] = serial
        rec = pending.pop(e, None)
        p_host = rec[0] if rec is not None and owner[rec[0]] == rec[1] else -1
        assert p_rule == p_host, (serial, e, w, rec)
        linked += p_host >= 0
        expired += rec is not None and p_host < 0
        for orc, p in ((by_rule, p_rule), (by_host, p_host)):
            assert orc.insert([float(serial)], [1.0], 0.0, 0, done, trunc, trunc or not done, p) == slot
        if not done and not trunc:
            tab[e] = serial
            pending[e] = (slot, serial)
        else:
            tab[e] = -1
        serial += 1
    np.testing.assert_array_equal(by_rule.link, by_host.link)
    assert linked > capacity and expired > 0                 # both outcomes were reached


def _sequential(link, back, owner, pending, serial0, first, cap, ids, is_open):
    """n one-row inserts as extend() + prism_replay_insert apply them: the host resolves each predecessor through the owner
    of its slot, then the row detaches the overwritten row's neighbours and attaches itself."""
    for i, e in enumerate(ids):
        s = (first + i) % cap
        owner[s] = serial0 + i
        rec = pending.pop(e, None)
        p = rec[0] if rec is not None and owner[rec[0]] == rec[1] else -1
        b, q = back[s], link[s]
        if b >= 0 and link[b] == s:
            link[b] = -1
        if q >= 0 and back[q] == s:
            back[q] = -1
        link[s] = back[s] = -1
        if p >= 0:
            link[p], back[s] = s, p
        if is_open[i]:
            pending[e] = (s, serial0 + i)


def _plan_phases(rng, link, back, tab, serial0, first, cap, ids, is_open):
    """ingest_kernels.h, plan workgroup, phase by phase (a workgroup barrier between phases; inside a phase the threads run
    in any order, here a random one): predecessor from the stream table, the test that picks the sequential fallback,
    phases A / B / C or the fallback loop, then the table update.  Returns whether the fallback ran."""
    n = len(ids)

    def pred_of(i):
        w = tab[ids[i]]
        if w < 0 or w >= serial0 + i or serial0 + i - w >= cap:
            return -1
        return int(w % cap)
    bad = any(p >= 0 and i <= (p - first + cap) % cap < n for i, p in ((i, pred_of(i)) for i in range(n)))
    slot = lambda i: (first + i) % cap
    if bad:
        for i in range(n):
            s = slot(i)
            b, q = back[s], link[s]
            if b >= 0 and link[b] == s:
                link[b] = -1
            if q >= 0 and back[q] == s:
                back[q] = -1
            link[s] = back[s] = -1
            p = pred_of(i)
            if p >= 0:
                link[p], back[s] = s, p
    else:
        for i in rng.permutation(n):                         # A
            s = slot(i)
            b, q = back[s], link[s]
            if b >= 0 and link[b] == s:
                link[b] = -1
            if q >= 0 and back[q] == s:
                back[q] = -1
        for i in rng.permutation(n):                         # B
            link[slot(i)] = back[slot(i)] = -1
        for i in rng.permutation(n):                         # C
            p = pred_of(i)
            if p >= 0:
                link[p], back[slot(i)] = slot(i), p
    for i in rng.permutation(n):                             # D
        tab[ids[i]] = serial0 + i if is_open[i] else -1
    return bad


def test_plan_phases_equal_the_sequential_loop():
    """The kernel's parallel plan restated on the host against n one-row inserts, over random rings (2 .. 39 slots), stream
    counts, subsets and orders per call: link and back agree after every call, on both the three-phase path and the
    sequential fallback (a predecessor overwritten later in the same call)."""
    rng = np.random.default_rng(0)
    fallbacks = parallel = 0
    for _ in range(400):
        cap, n_streams = int(rng.integers(2, 40)), int(rng.integers(1, 12))
        l1, b1, l2, b2 = (np.full(cap, -1) for _ in range(4))
        owner, pending, tab, serial = np.full(cap, -1), {}, np.full(n_streams, -1, np.int64), 0
        for _ in range(30):
            n = int(rng.integers(1, min(n_streams, cap) + 1))
            ids = [int(x) for x in rng.permutation(n_streams)[:n]]
            is_open = rng.random(n) < 0.85
            first = serial % cap
            _sequential(l1, b1, owner, pending, serial, first, cap, ids, is_open)
            bad = _plan_phases(rng, l2, b2, tab, serial, first, cap, ids, is_open)
            fallbacks, parallel = fallbacks + bad, parallel + (not bad)
            serial += n
            np.testing.assert_array_equal(l1, l2)
            np.testing.assert_array_equal(b1, b2)
    assert fallbacks > 100 and parallel > 100
