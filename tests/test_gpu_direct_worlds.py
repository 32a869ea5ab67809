"""GPU: the direct all-reduce (prism_amd/csrc/direct.hip) at worlds 1..8, on ONE device in ONE process.

A rank is nothing but a descriptor: W descriptors over W buffers of one device, launched one after the other on one
stream, run exactly the code W devices would -- the summation order, ``slice_range`` at lengths W does not divide, empty
slices, the tail, ``flags[t] + rank`` for more than one peer.  The expected value is ``tests/direct_ref.ordered_sum``
(float32 adds in rank order), compared by bit pattern; tests/test_direct_host.py shows that on these inputs another order
gives other bits in every slice and every tail element.  No kernel here ever spins on a peer that has yet to run: waits are
launched behind the announcements they look for, or are the 0.2 s bounded give-up of the time-out tests.

Every buffer lies between two rows of 64 guard floats, which must come through every test untouched."""
import ctypes
import os

import numpy as np
import pytest
import torch

from tests import direct_cases as C
from tests import direct_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GUARD = 64
GUARD_BITS = 0x7FC5A5A5          # a NaN no sum produces


@pytest.fixture(scope="module")
def N():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from prism_amd import _native
    _native.lib()
    return _native


class Ranks:
    """W guarded buffers on one device and a descriptor per rank over them; optionally W flag arrays every descriptor
    sees, and a poison word plus pinned status words per rank."""

    def __init__(self, N, bufs, flags=False, wait_seconds=0.2):
        from prism_amd import dist as pdist
        self.N, self.W, self.n = N, len(bufs), int(bufs[0].shape[0])
        self.alloc, self.payload = [], []
        for b in bufs:
            a = torch.full((GUARD + self.n + GUARD,), GUARD_BITS, dtype=torch.int32, device=DEV).view(torch.float32)
            p = a[GUARD:GUARD + self.n]
            p.copy_(torch.from_numpy(np.array(b)))
            assert p.data_ptr() % 16 == 0
            self.alloc.append(a)
            self.payload.append(p)
        self.flag_ptrs = []
        if flags:
            for _ in range(self.W):
                fp = ctypes.c_void_p(0)
                N.check(N.lib().prism_direct_flags_alloc(ctypes.byref(fp), None), "prism_direct_flags_alloc")
                self.flag_ptrs.append(fp.value)
        self.poison = torch.zeros(self.W, dtype=torch.int32, device=DEV)
        self.status = [pdist.StatusWords() for _ in range(self.W)]
        self.desc = []
        for r in range(self.W):
            d = N.DirectDesc()
            d.world, d.rank, d.n, d.wait_seconds = self.W, r, self.n, wait_seconds          # every wait is bounded
            for s in range(self.W):
                d.bufs[s] = self.payload[s].data_ptr()
                if flags:
                    d.flags[s] = self.flag_ptrs[s]
            if flags:
                d.poison, d.host_status = self.poison.data_ptr() + 4 * r, self.status[r].data_ptr()
            self.desc.append(d)

    def _call(self, name, r, *args):
        N = self.N
        N.check(getattr(N.lib(), name)(ctypes.byref(self.desc[r]), *args, N.current_stream_handle()), name)

    def reduce_scatter(self, r, use_flags=0):
        self._call("prism_direct_reduce_scatter", r, use_flags)

    def all_gather(self, r, use_flags=0):
        self._call("prism_direct_all_gather", r, use_flags)

    def phase(self, r, phase, what):
        self._call("prism_direct_phase", r, phase, what)

    def paced_allreduce(self, ranks=None, salt=0, first_announced=False):
        """One all-reduce of `ranks` (default: all) through the flag kernels, paced on the stream: per phase every rank
        announces, then every rank waits -- a wait finds its flags set -- with the use_flags = 0 kernels in between."""
        ranks = list(range(self.W)) if ranks is None else ranks
        order = [r for r in C.launch_order(self.W, salt) if r in ranks]
        for ph, work in ((1, self.reduce_scatter), (2, self.all_gather), (3, None)):
            if not (ph == 1 and first_announced):
                for r in order:
                    self.phase(r, ph, 1)
            for r in reversed(order):
                self.phase(r, ph, 2)
            if work is not None:
                for r in order:
                    work(r)

    def read(self):
        torch.cuda.synchronize()
        return [p.cpu().numpy() for p in self.payload]

    def flags(self, r):
        N = self.N
        out = (ctypes.c_uint32 * N.DIRECT_FLAG_WORDS)()
        N.check(N.lib().prism_direct_flags_read(self.flag_ptrs[r], out, N.current_stream_handle()), "prism_direct_flags_read")
        return list(out)

    def check_guards(self):
        torch.cuda.synchronize()
        for a in self.alloc:
            g = a.view(torch.int32)
            assert bool((g[:GUARD] == GUARD_BITS).all()) and bool((g[GUARD + self.n:] == GUARD_BITS).all()), "guard floats overwritten"

    def close(self):
        torch.cuda.synchronize()
        for p in self.flag_ptrs:
            self.N.check(self.N.lib().prism_direct_flags_free(p), "prism_direct_flags_free")
        self.flag_ptrs = []


def same_bits(got, want, what):
    g, w = R.bits(got), R.bits(want)
    bad = np.flatnonzero(g != w)
    assert bad.size == 0, f"{what}: {bad.size} of {g.size} floats differ, first at {bad[:8].tolist()}"


# ---- a. the host-paced form ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,n", C.CASES + (C.CLAMP_CASE,), ids=lambda v: str(v))
def test_reduce_scatter_then_all_gather_in_rank_order(N, W, n):
    bufs, want = C.inputs(W, n)
    rk = Ranks(N, bufs)
    for r in C.launch_order(W, salt=n):
        rk.reduce_scatter(r)
    got = rk.read()
    for r in range(W):
        # the ordered sum on what rank r owns (the last rank: the tail too), its own values everywhere else
        same_bits(got[r], R.after_reduce_scatter(bufs, r), f"W={W} n={n}: buffer {r} after the reduce-scatter")
    for r in C.launch_order(W, salt=n + 1):
        rk.all_gather(r)
    got = rk.read()
    for r in range(W):
        same_bits(got[r], want, f"W={W} n={n}: buffer {r} after the all-gather")
    rk.check_guards()


# ---- b. the device-flag protocol, paced on one stream --------------------------------------------------------------------
@pytest.mark.parametrize("W", [3, 5, 8])
@pytest.mark.parametrize("which", ["one float4", "blocks and tail"])
def test_flag_protocol_eager_and_replayed(N, W, which):
    from prism_amd.agents.hip_agent import graph_capture
    n = 7 if which == "one float4" else 4 * (256 * W + 1) + 1
    bufs, _ = C.inputs(W, n)
    rk = Ranks(N, bufs, flags=True)
    try:
        s = torch.cuda.Stream()
        with torch.cuda.stream(s):
            rk.paced_allreduce(salt=1)
            rk.paced_allreduce(salt=2)
            for r in range(W):
                f = rk.flags(r)
                assert f[N.MAX_PEERS + 1] == 2 and f[:W] == [3 * 1 + 3] * W and f[N.MAX_PEERS] == 0, (r, f)
            g = torch.cuda.CUDAGraph()
            with graph_capture(g):          # one chain on the capture stream: no branch, no side stream
                rk.paced_allreduce(salt=3)
            for _ in range(3):
                g.replay()
            for r in range(W):
                f = rk.flags(r)
                assert f[N.MAX_PEERS + 1] == 5, (r, f)                          # epoch
                assert f[:W] == [3 * 4 + 3] * W, (r, f)                         # every peer's last announcement
                assert f[W:N.MAX_PEERS] == [0] * (N.MAX_PEERS - W), (r, f)      # nobody wrote a slot past the world
                assert f[N.MAX_PEERS] == 0, (r, f)                              # no wait gave up
        torch.cuda.synchronize()
        assert rk.poison.cpu().tolist() == [0] * W and all(st.bits() == 0 for st in rk.status)
        want = R.iterated(bufs, 5)
        for r, got in enumerate(rk.read()):
            same_bits(got, want, f"W={W} n={n}: buffer {r} after five all-reduces")
        rk.check_guards()
    finally:
        rk.close()


# ---- c. a rank that gives up takes its peers with it ---------------------------------------------------------------------
@pytest.mark.parametrize("gives_up_in", [1, 2])
def test_timeout_of_one_rank_poisons_every_rank(N, gives_up_in):
    """World 3; rank 0 runs the step's real form (announce + bounded wait in one launch, 0.2 s) when its peers have not
    arrived -- before anyone has announced anything (it gives up in phase 1), or when they have announced phase 1 only (it
    reduces its slice and gives up in phase 2).  Ranks 1 and 2 then run the rest, paced.  None of their waits gives up, and
    still every rank must end poisoned: a peer of a rank that gave up would otherwise gather that rank's un-reduced slice and
    run clip + Adam on it."""
    W, n = 3, 4 * (256 * 3 + 1) + 1
    bufs, want = C.inputs(W, n)
    rk = Ranks(N, bufs, flags=True, wait_seconds=0.2)
    try:
        if gives_up_in == 2:
            rk.phase(1, 1, 1)
            rk.phase(2, 1, 1)
        rk.reduce_scatter(0, use_flags=1)
        rk.all_gather(0, use_flags=1)
        rk.paced_allreduce(ranks=[1, 2], first_announced=gives_up_in == 2)
        torch.cuda.synchronize()
        T = N.WS_STATUS_COLLECTIVE_TIMEOUT
        assert rk.poison.cpu().tolist() == [T] * W                               # every rank's step is poisoned on the device,
        assert [st.bits() for st in rk.status] == [T] * W                        # every rank's host sees it without a sync,
        sticky = [rk.flags(r)[N.MAX_PEERS] for r in range(W)]
        assert all(v != 0 for v in sticky), sticky                               # and every rank's reduce kernels are off
        first = rk.read()
        for r in range(W):
            lo, hi = R.float_range(n, W, r)
            keep = np.ones(n, bool)
            keep[lo:hi] = False
            # nobody gathered anything: outside its own slice every buffer is what it was
            assert (R.bits(first[r])[keep] == R.bits(bufs[r])[keep]).all(), f"buffer {r} was written outside its own slice"
        lo, hi = R.float_range(n, W, 0)
        if gives_up_in == 2:          # rank 0 got through phase 1: its slice is reduced, and correctly
            assert (R.bits(first[0])[lo:hi] == R.bits(want)[lo:hi]).all()
        else:
            same_bits(first[0], bufs[0], "buffer 0")
        # a second all-reduce by all three: nothing moves any more
        rk.paced_allreduce(salt=5)
        for r, got in enumerate(rk.read()):
            same_bits(got, first[r], f"buffer {r} after a second all-reduce of poisoned ranks")
        assert [rk.flags(r)[N.MAX_PEERS + 1] for r in range(W)] == [2] * W       # (the epochs still advance in lockstep)
        rk.check_guards()
    finally:
        rk.close()


# ---- d. three processes, once -------------------------------------------------------------------------------------------
WORLD3_SIZES = (7, 4099, 201_430)


def _world3_worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    from prism_amd import dist as pdist
    ok = True
    for n in WORLD3_SIZES:
        mine = np.array(C.inputs(world, n)[0][rank])
        flat = torch.from_numpy(mine).to(DEV)
        everyone = [torch.zeros(n) for _ in range(world)]
        dist.all_gather(everyone, torch.from_numpy(mine))          # the inputs travel over gloo; the SUM is ours: gloo's order is not promised
        want = R.ordered_sum([e.numpy() for e in everyone])
        ar = pdist.DirectAllReduce(flat, wait_seconds=5.0)
        assert ar.use_flags is False and not ar.paced               # three ranks on ONE device: host barriers, no device spinning
        ok = ok and len({ar._desc.bufs[s] for s in range(world)}) == world and ar._desc.bufs[rank] == flat.data_ptr()
        ok = ok and len({ar._desc.flags[s] for s in range(world)}) == world and ar._desc.flags[rank] == ar._flags_ptr
        scale = ar.allreduce()
        torch.cuda.synchronize()
        ar.check_status()
        ok = ok and scale == 1.0 / world and bool((R.bits(flat.cpu().numpy()) == R.bits(want)).all())
        dist.barrier()
        ar.close()
        del ar
    q.put((rank, ok))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_three_processes_sum_in_rank_order(N):
    """World 3 through ``dist.DirectAllReduce``: torch's IPC mapping of the gradient buffers and the library's flag handles
    with two peers per rank, three processes on the one device with host barriers between the phases."""
    import torch.multiprocessing as mp
    from tests.test_gpu_dp import _free_port
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_world3_worker, args=(r, 3, port, q)) for r in range(3)]
    for p in procs:
        p.start()
    try:
        res = [q.get(timeout=240) for _ in procs]
        for p in procs:
            p.join(60)
            assert p.exitcode == 0
    finally:
        for p in procs:
            if p.is_alive():
                p.kill()
    assert sorted(res) == [(0, True), (1, True), (2, True)]
