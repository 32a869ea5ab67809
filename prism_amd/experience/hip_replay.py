"""HBM-resident replay ring with prioritized sum/min trees — duck-types the reference's
``TimestepBuffer`` (``/root/reference/prism/experience/timestep_buffer.py:10-77``) and the torchrl
buffer it wraps (``prism/factory/exp_buffer_factory.py:22-33``).

Data layout (all device memory, allocated once, sized for 288 GB of HBM3E):
    obs, succ_obs  fp32 [capacity, O]     reward fp32 [capacity]      action int32 [capacity]
                   (``obs_storage="uint8"``: uint8 [capacity, O], a quarter of the bytes, for byte-exact observations)
    flags uint8 [capacity]                link/back int32 [capacity]
    tree fp32 [2 * tree_capacity][2]  ({sum, min} per node; sum_tree / min_tree are views)
Python ``Timestep`` objects are consumed at ``extend()`` and not kept.  ``sample()`` runs two
kernels (tree descent + IS weights; n-step walk + row gather) and returns the reference's static
batch layout without any host loop or H2D copy.
"""
import ctypes
import os
import pickle
import weakref

import numpy as np
import torch

from prism_amd import _native as N


class Batch(dict):
    """Nested dict of device tensors with the bits of TensorDict the learner touches
    (``learner.py:71`` ``.clone()``, ``agent.py:105`` ``.device``)."""

    def __init__(self, d=None, batch_size=None, device=None):
        super().__init__(d or {})
        self.batch_size, self.device = batch_size, device

    def clone(self):
        out = Batch({}, self.batch_size, self.device)
        for k, v in self.items():
            out[k] = v.clone()
        return out


class _SamplerShim:
    """``buffer.buffer._sampler`` — the learner writes ``_beta`` every step (learner.py:107)."""

    def __init__(self, alpha, beta, eps=1e-8):
        self._alpha, self._beta, self._eps = float(alpha), float(beta), float(eps)


class _WriterShim:
    def __init__(self):
        self._cursor = 0


class _RingShim:
    """``buffer.buffer`` — the attribute chain the reference reaches through."""

    def __init__(self, owner, batch_size, alpha, beta):
        self._owner = owner
        self._batch_size = batch_size
        self._sampler = _SamplerShim(alpha, beta)
        self._writer = _WriterShim()
        self._storage = owner          # len(buffer.buffer._storage)

    def __len__(self):
        return len(self._owner)


class _Staging:
    """Two sets of pinned host blocks with their device twins, in rotation: the host fills one while the copies and the
    kernel that read the other are still in flight.  An event recorded behind the launch that reads a set guards it, and
    is waited for only when that set comes round again -- a whole submission later."""

    def __init__(self, make_set):
        self.sets, self._ev, self._cur = (make_set(), make_set()), [None, None], 0

    def acquire(self):
        """The set to fill next; waits only if the launch that last read it has not finished."""
        ev = self._ev[self._cur]
        if ev is not None:
            ev.synchronize()
            self._ev[self._cur] = None
        return self.sets[self._cur]

    def submit(self):
        """Behind the launch that reads the current set (same device, same stream): guard it and turn to the other."""
        self._ev[self._cur] = ev = torch.cuda.Event()
        ev.record()
        self._cur ^= 1

    def drain(self):
        """Before the sets are dropped: nothing in flight reads them any more."""
        for ev in self._ev:
            if ev is not None:
                ev.synchronize()


_SMALL_INT = {True: (torch.bool, torch.uint8), False: (np.bool_, np.uint8)}       # observation dtypes stored as uint8
# obs_storage -> (ring kind of the prism_*_ring entry points, dtype of obs / succ_obs)
_OBS_STORAGE = {"float32": (N.RING_F32, torch.float32), "uint8": (N.RING_U8, torch.uint8)}


def _as_u8(x):
    return x.clamp(0, 255).to(torch.uint8)


def _byte_exact(x):
    """Every value of the float32 tensor is BYTE-EXACT -- the bit pattern of float(b) for a b in 0..255 (so not -0.0, NaN,
    a fraction, a negative, above 255): a 0-d bool tensor, compared in bit space (common.h obs_narrow)."""
    x = x.contiguous()
    return (_as_u8(x).to(torch.float32).view(torch.int32) == x.view(torch.int32)).all()


def _narrow_host(x, what):
    """A host observation array as the bytes a uint8 ring stores; a value that is not byte-exact is a ValueError."""
    x = np.asarray(x)
    if x.dtype in _SMALL_INT[False]:
        return x.astype(np.uint8, copy=False)
    f = np.ascontiguousarray(x, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        b = np.where((f >= 0) & (f <= 255), f, np.float32(0)).astype(np.uint8)
    if not np.array_equal(b.astype(np.float32).view(np.uint32), f.view(np.uint32)):
        raise ValueError(f"{what}: obs_storage='uint8' holds only byte-exact observations (+0.0, 1.0 .. 255.0); "
                         "nothing was written")
    return b


def _is_dev(x):
    return torch.is_tensor(x) and x.is_cuda


def _host(x):
    return x.numpy() if torch.is_tensor(x) else np.asarray(x)


def _obs_kind(obs, next_obs):
    """OBS_U8 / OBS_F32 of one extend_batch call: both observation arrays small-int (bool / uint8) or both float."""
    small = [x.dtype in _SMALL_INT[torch.is_tensor(x)] for x in (obs, next_obs)]
    if small[0] != small[1]:
        raise ValueError(f"extend_batch: obs ({obs.dtype}) and next_obs ({next_obs.dtype}) must both be bool / uint8 "
                         "or both be floating point")
    return N.OBS_U8 if small[0] else N.OBS_F32


def _check_stream_ids(stream_ids, n, table_size):
    """The stream ids of one extend_batch call, checked as far as the host can without touching a device: (the ids as a
    host array, or None for device-side / default ids; the number of table entries the call needs)."""
    if stream_ids is None:
        return None, n
    if _is_dev(stream_ids):
        if stream_ids.numel() != n:
            raise ValueError("extend_batch: stream_ids must hold one id per row")
        return None, max(n, table_size)
    ids = _host(stream_ids).reshape(-1)
    if ids.shape[0] != n:
        raise ValueError("extend_batch: stream_ids must hold one id per row")
    if int(ids.min()) < 0 or int(ids.max()) >= N.INGEST_MAX_STREAMS:
        raise ValueError(f"extend_batch: stream_ids must lie in [0, {N.INGEST_MAX_STREAMS})")
    seen = np.zeros(int(ids.max()) + 1, np.bool_)
    seen[ids] = True
    if int(seen.sum()) != n:
        raise ValueError("extend_batch: stream_ids must be distinct within one call")
    return ids, seen.shape[0]


def _device_array(x, shape, dtype, stage):
    """`x` as a contiguous device array of `dtype`, and whether it went through staging.  A device tensor is used in place
    (bool is viewed as uint8, any other dtype bound for uint8 becomes x != 0, the rest is converted); anything else is
    written into `stage` = (NumPy view of a pinned block, the same bytes of its device twin), which the caller copies."""
    if not _is_dev(x):
        np.copyto(stage[0], _host(x).reshape(shape), casting="unsafe")
        return stage[1], True
    x = x.reshape(shape)
    if dtype == torch.uint8 and x.dtype != torch.uint8:
        x = x.view(torch.uint8) if x.dtype == torch.bool else (x != 0).view(torch.uint8)
    return (x if x.dtype == dtype else x.to(dtype)).contiguous(), False


class HipReplayBuffer:
    STAGE_ROWS = 1024

    def __init__(self, capacity, batch_size, device="cuda:0", frame_stack=1, n_step=3, gamma=0.99,
                 use_per=True, alpha=0.5, beta=0.5, mass_rng="philox", seed=123, strict=False, reward_clipping_type=None,
                 obs_storage="float32"):
        if obs_storage not in _OBS_STORAGE:
            raise ValueError(f"obs_storage = {obs_storage!r} must be one of {sorted(_OBS_STORAGE)}")
        if frame_stack != 1:
            raise NotImplementedError("prism_amd replay: frame_stack_size > 1 is not implemented")
        if not str(device).startswith("cuda"):
            raise N.NativeLibraryError("HipReplayBuffer needs a GPU device; there is no CPU fallback")
        if not 1 <= n_step <= N.PRISM_MAX_NSTEP:
            raise ValueError("n_step out of range")
        N.lib()
        self.device = torch.device(device)
        self.capacity = int(capacity)
        self.tree_capacity = 1
        while self.tree_capacity <= self.capacity:
            self.tree_capacity <<= 1
        self.frame_stack, self.n_step, self.gamma = frame_stack, int(n_step), float(gamma)
        self.gammas = [gamma ** i for i in range(n_step + 1)]
        self.use_per = bool(use_per)
        self.mass_rng, self.seed, self.strict = mass_rng, int(seed), bool(strict)
        self.buffer = _RingShim(self, batch_size, alpha, beta)
        # storage kind of obs / succ_obs: fp32 (the reference layout), or one byte per element for byte-exact observations
        # (MinAtar's boolean planes): a uint8 ring fed them is bit for bit the fp32 ring at a quarter of the HBM
        self.obs_storage = obs_storage
        self._ring_kind, self._obs_dtype = _OBS_STORAGE[obs_storage]
        self._size = 0
        self._draws = 0            # Philox counters consumed by sample() (host-issued offsets)
        self._fused_draws = 0      # ... and by fused steps (device counter; mirrored here so the two never overlap)
        self._obs_shape = None
        self._desc = None
        self._batch = None
        self._pending = {}        # successor Timestep.id -> (slot, id) of the stored predecessor
        self._slot_id = np.full(self.capacity, -1, np.int64)
        self._n_staged = 0
        self._index = None
        # vectorised producer seam (extend_batch): rows ever written since init / empty / bulk load (serial % capacity ==
        # writer cursor), the device table "write serial of each stream's open row", and its staging rotation
        self._serial = 0
        self._stream_tab = None
        self._ing = None
        # ... its reward clip, compared as collector_process_interface.py:136-139 compares it ("dopamine_clamp" clamps,
        # "sign" divides by zero there, every other value -- DEFAULT_CONFIG's "dopamine_clip" included -- clips nothing),
        # and the episode bookkeeping track_episodes() turns on: per-stream accumulators as long as the stream table
        self.reward_clipping_type = reward_clipping_type
        self._clip = N.CLIP_CLAMP if reward_clipping_type == "dopamine_clamp" else N.CLIP_NONE
        self._ep = None            # dict(ema, count_first_step) while tracking
        self._ep_return = self._ep_length = self._ep_words = self._ep_stats = self._ep_counts = None
        self._ep_desc = self._ep_desc_ref = None
        # the cursor form of extend_batch (a captured launch): the two device words, and (slot, value) the host knows one of
        # them to hold -- None or stale after anything else has moved the count
        self._cursor_words = None
        self._cursor_known = None

    # ------------------------------------------------------------------ allocation
    def _allocate(self, obs_shape):
        """Step a of every bulk install, and of the first extend: the ring for this observation shape, empty -- allocated
        now, or (a load into a buffer that has been used) brought back to the state of a fresh one."""
        if self._desc is not None:
            for t in (self.obs, self.succ_obs, self.reward, self.action):      # (empty() leaves the rows' payload behind)
                t.zero_()
            return self.empty()
        dev, cap = self.device, self.capacity
        self._obs_shape = tuple(int(s) for s in obs_shape)
        O = int(np.prod(self._obs_shape))
        self.obs_elems = O
        self.obs = torch.zeros(cap, O, dtype=self._obs_dtype, device=dev)
        self.succ_obs = torch.zeros(cap, O, dtype=self._obs_dtype, device=dev)
        self.reward = torch.zeros(cap, dtype=torch.float32, device=dev)
        self.action = torch.zeros(cap, dtype=torch.int32, device=dev)
        self.flags = torch.zeros(cap, dtype=torch.uint8, device=dev)
        self.link = torch.full((cap,), -1, dtype=torch.int32, device=dev)
        self.back = torch.full((cap,), -1, dtype=torch.int32, device=dev)
        if self.use_per:
            # {sum, min} of a node side by side: one 16-byte load yields both children of a node
            self.tree = torch.zeros(2 * self.tree_capacity, 2, dtype=torch.float32, device=dev)
            self.sum_tree, self.min_tree = self.tree[:, 0], self.tree[:, 1]      # strided views
        else:
            self.tree = self.sum_tree = self.min_tree = None
        self.per_state = torch.zeros(4, dtype=torch.float32, device=dev)
        self.status = torch.zeros(1, dtype=torch.int32, device=dev)
        d = N.ReplayDesc()
        d.capacity, d.tree_capacity, d.obs_elems, d.n_step = cap, self.tree_capacity, O, self.n_step
        for name in ("obs", "succ_obs", "reward", "action", "flags", "link", "back", "tree",
                     "per_state", "status"):
            t = getattr(self, name)
            setattr(d, name, t.data_ptr() if t is not None else None)
        for i, g in enumerate(self.gammas):
            d.gammas[i] = g
        self._desc, self._desc_ref = d, ctypes.byref(d)
        self._on_device = torch.cuda.device(dev)         # entered around every native call (_call; never nested)
        self._call("prism_replay_init")
        # staging (pinned host -> device) for extend(): a _Staging rotation of two sets.
        # The five per-row scalars live side by side in ONE pinned block (and one device block): a flush is three
        # host-to-device copies -- that block whole (17 bytes a row), the used observation rows, the used successor rows --
        # instead of seven.  extend() writes through NumPy views of the pinned memory (a torch scalar store costs 2 us),
        # bound to plain attributes (_h, _d, _hn) at rotation time: the per-row body pays for no call and no lookup chain.
        S = self.STAGE_ROWS

        def _blocks(**kw):
            small = torch.zeros(17 * S, dtype=torch.uint8, **kw)      # slots | reward | action | prev (4 bytes each) | flags (1)
            w = lambda k: small[4 * S * k:4 * S * (k + 1)]
            return dict(small=small, slots=w(0).view(torch.int32), reward=w(1).view(torch.float32),
                        action=w(2).view(torch.int32), prev=w(3).view(torch.int32), flags=small[16 * S:],
                        obs=torch.zeros(S, O, dtype=self._obs_dtype, **kw), succ=torch.zeros(S, O, dtype=self._obs_dtype, **kw))

        def _set():
            h, d = _blocks(pin_memory=True), _blocks(device=dev)
            # (the device twins never move: prism_replay_insert's seven array arguments are made once)
            args = tuple(N.ptr(d[k]) for k in ("slots", "obs", "succ", "reward", "action", "flags", "prev"))
            return dict(h=h, d=d, np={k: v.numpy() for k, v in h.items()}, args=args)
        self._row_stage = _Staging(_set)
        self._bind_row_stage()
        self._alloc_batch(self.buffer._batch_size)

    def _bind_row_stage(self):
        st = self._row_stage.acquire()
        self._h, self._d, self._hn, self._insert_args = st["h"], st["d"], st["np"], st["args"]

    def _alloc_batch(self, B):
        dev, fs = self.device, self.frame_stack
        shp = (B, fs) + self._obs_shape
        batch = Batch({
            "observation": torch.zeros(shp, dtype=torch.float32, device=dev),
            "next": Batch({"observation": torch.zeros(shp, dtype=torch.float32, device=dev),
                           "reward": torch.zeros(B, 1, dtype=torch.float32, device=dev)}, B, dev),
            "nonterminal": torch.zeros(B, 1, dtype=torch.bool, device=dev),
            "gamma": torch.ones(B, 1, dtype=torch.float32, device=dev),
            "action": torch.zeros(B, 1, dtype=torch.long, device=dev)}, B, dev)
        self.set_static_batch(batch)
        self._index = torch.zeros(B, dtype=torch.int64, device=dev)
        self._weight = torch.ones(B, dtype=torch.float32, device=dev)
        self._mass = torch.zeros(B, dtype=torch.float32, device=dev)
        self._q2 = torch.zeros(2, dtype=torch.float32, device=dev)

    def _call(self, name, *args, desc=True, submit=None):
        """One native call on this buffer's device and its current stream: the ring descriptor in front (desc=False:
        the entry point takes none), the stream behind, the return code checked.  `submit`: the staging rotation whose
        current set the launch reads, guarded and turned right behind it."""
        with self._on_device:
            head = (self._desc_ref,) if desc else ()
            N.check(getattr(N.lib(), name)(*head, *args, N.current_stream_handle()), name)
            if submit is not None:
                submit.submit()

    # ------------------------------------------------------------------ reference API
    def __len__(self):
        return self._size

    def extend(self, timestep):
        """TimestepBuffer.extend (timestep_buffer.py:32-33): one completed timestep."""
        rows = None
        if self._ring_kind:                            # byte ring: an inexact observation is refused before anything changes
            nxt = timestep.next
            node = (nxt() if isinstance(nxt, weakref.ReferenceType) else nxt) if nxt is not None else None
            rows = (_narrow_host(timestep.obs, "extend").reshape(-1),
                    0 if node is None else _narrow_host(node.obs, "extend").reshape(-1))
        if self._desc is None:
            self._allocate(tuple(timestep.obs.shape))
        if self._n_staged == self.STAGE_ROWS:
            self.flush()
        w = self.buffer._writer
        s = w._cursor
        w._cursor = (s + 1) % self.capacity
        self._size = min(self._size + 1, self.capacity)
        self._slot_id[s] = timestep.id
        self._serial += 1

        prev_slot = -1
        rec = self._pending.pop(timestep.id, None)
        if rec is not None and self._slot_id[rec[0]] == rec[1]:
            prev_slot = rec[0]
        nxt = timestep.next
        node = None
        if nxt is not None:
            node = nxt() if isinstance(nxt, weakref.ReferenceType) else nxt
        flags = (N.FLAG_DONE if timestep.done else 0) | (N.FLAG_TRUNC if timestep.truncated else 0) | \
                (N.FLAG_HAS_NEXT if node is not None else 0)
        if node is not None and isinstance(nxt, weakref.ReferenceType) and not timestep.truncated:
            self._pending[node.id] = (s, timestep.id)

        i, h = self._n_staged, self._hn
        h["slots"][i] = s
        if rows is not None:
            h["obs"][i], h["succ"][i] = rows
        else:
            h["obs"][i] = np.asarray(timestep.obs, dtype=np.float32).reshape(-1)
            if node is not None:
                h["succ"][i] = np.asarray(node.obs, dtype=np.float32).reshape(-1)
            else:
                h["succ"][i] = 0.0
        h["reward"][i] = timestep.reward
        h["action"][i] = timestep.action
        h["flags"][i] = flags
        h["prev"][i] = prev_slot
        self._n_staged += 1
        return s

    def flush(self):
        """Push staged rows into the HBM ring (one H2D batch + two small kernels)."""
        n = self._n_staged
        if n == 0:
            return
        h, d, smp = self._h, self._d, self.buffer._sampler
        d["small"].copy_(h["small"], non_blocking=True)
        d["obs"][:n].copy_(h["obs"][:n], non_blocking=True)
        d["succ"][:n].copy_(h["succ"][:n], non_blocking=True)
        if self._ring_kind:                            # (uint8 row staging, copied into the byte ring)
            a = self._insert_args
            self._call("prism_replay_insert_ring", self._ring_kind, n, *a[:3], N.OBS_U8, *a[3:], smp._alpha, smp._eps,
                       submit=self._row_stage)
        else:
            self._call("prism_replay_insert", n, *self._insert_args, smp._alpha, smp._eps, submit=self._row_stage)
        self._bind_row_stage()         # the other set takes the next rows; it was submitted a whole batch ago
        self._n_staged = 0

    # ------------------------------------------------------------------ vectorised producer seam
    def _stream_table(self, need):
        """The device stream table, grown (doubling, -1 = no open row) to hold at least `need` streams."""
        if need > N.INGEST_MAX_STREAMS:
            raise ValueError(f"extend_batch: stream_ids must lie in [0, {N.INGEST_MAX_STREAMS})")
        t = self._stream_tab
        if t is None or t.numel() < need:
            size = 64
            while size < need:
                size <<= 1
            new = torch.full((size,), -1, dtype=torch.int64, device=self.device)
            if t is not None:
                new[:t.numel()].copy_(t)
            self._stream_tab = new
            self._fit_episode_arrays()
        return self._stream_tab

    # ------------------------------------------------------------------ reward clip + episode returns on the device
    def _fit_episode_arrays(self):
        """The per-stream accumulators, as long as the stream table: old entries kept, the rest zero."""
        if self._ep is None:
            return
        size = self._stream_tab.numel()
        if self._ep_return is None or self._ep_return.numel() != size:
            ret = torch.zeros(size, dtype=torch.float64, device=self.device)
            length = torch.zeros(size, dtype=torch.int32, device=self.device)
            if self._ep_return is not None:
                k = min(size, self._ep_return.numel())
                ret[:k].copy_(self._ep_return[:k])
                length[:k].copy_(self._ep_length[:k])
            self._ep_return, self._ep_length = ret, length
        self._bind_episode_desc()

    def _bind_episode_desc(self):
        """What prism_replay_ingest_tracked takes besides prism_replay_ingest's arguments (made anew when an array moves)."""
        d = N.EpisodeDesc()
        d.reward_clip = self._clip
        if self._ep is not None:
            d.count_first_step, d.ema = int(self._ep["count_first_step"]), self._ep["ema"]
            d.ep_return, d.ep_length = self._ep_return.data_ptr(), self._ep_length.data_ptr()
            d.stats, d.counts = self._ep_stats.data_ptr(), self._ep_counts.data_ptr()
        self._ep_desc, self._ep_desc_ref = d, ctypes.byref(d)

    def track_episodes(self, ema=0.9, count_first_step=False):
        """Keep, on the device and inside extend_batch's one launch, what the reference's collector keeps per timestep
        (collector_process_interface.py:129-133, experience_collector.py:113-118): every stream's episodic return over the
        RAW rewards, in float64, and the training reward -- the EMA over the returns of finished episodes, folded in row
        order.  ``count_first_step=False`` is the reference's rule: the first reward of an episode is not counted (a
        one-step episode reports 0).  Rows that arrive through ``extend()`` are not tracked.  Read with ``episode_stats()``."""
        ema, count_first_step = float(ema), bool(count_first_step)
        if not (np.isfinite(ema) and 0.0 <= ema <= 1.0):
            raise ValueError(f"track_episodes: ema = {ema} must lie in [0, 1]")
        if self._ep is not None:
            if self._ep != dict(ema=ema, count_first_step=count_first_step):
                raise ValueError(f"track_episodes: already tracking with {self._ep}; the parameters cannot change")
            return
        N.lib()
        with torch.cuda.device(self.device):
            self._ep = dict(ema=ema, count_first_step=count_first_step)
            # stats (float64 [4]) and counts (int64 [4]) side by side: episode_stats() is ONE device-to-host copy
            self._ep_words = torch.zeros(8, dtype=torch.int64, device=self.device)
            self._ep_stats, self._ep_counts = self._ep_words[:4].view(torch.float64), self._ep_words[4:]
            self._stream_table(1)
            self._fit_episode_arrays()

    def episode_stats(self):
        """The finished-episode statistics of the tracked rows so far (one small device-to-host copy: for report time).
        ``training_reward`` is None until the first episode has ended, as the reference logs it."""
        if self._ep is None:
            raise RuntimeError("episode_stats: call track_episodes() first")
        w = self._ep_words.cpu()
        stats, counts = w[:4].view(torch.float64).tolist(), w[4:].tolist()
        n = int(counts[0])
        some = n > 0
        return dict(episodes=n, training_reward=stats[0] if some else None, mean_return=stats[1] / n if some else None,
                    mean_length=counts[1] / n if some else None, last_return=stats[2] if some else None,
                    rows=int(counts[2]))

    def _close_episodes(self):
        """No stream has an open episode any more; what finished episodes have added up stays."""
        if self._ep is not None:
            self._ep_return.zero_()
            self._ep_length.zero_()

    def reserve_streams(self, n_streams):
        """Size the stream table for ids 0 .. n_streams - 1 ahead of time.  Needed only with DEVICE-side ``stream_ids``:
        the host cannot read them without a sync, so the table cannot grow on their demand (host-side ids and the default
        numbering grow it by themselves); a device-side id at or above the table's size is stored unlinked and sets the
        sticky status bit."""
        if not 1 <= int(n_streams) <= N.INGEST_MAX_STREAMS:
            raise ValueError(f"reserve_streams: n_streams must be in [1, {N.INGEST_MAX_STREAMS}]")
        with torch.cuda.device(self.device):
            self._stream_table(int(n_streams))

    def _ingest_views(self, n, kind):
        """The staging set the next extend_batch fills (a _Staging rotation, regrown to a power of two of rows when a call
        needs more) as views for `n` rows of observation kind `kind`, cached per (n, kind): key -> (NumPy view of the
        pinned block, the same bytes of the device twin), and ``copies``: block -> (device twin, pinned block) in use."""
        O = self.obs_elems
        if self._ing is None or self._ing.sets[0]["rows"] < n:
            if self._ing is not None:
                self._ing.drain()
            rows = 64
            while rows < n:
                rows <<= 1
            # observations as raw bytes (viewed fp32 or uint8); the five per-row scalars side by side in ONE block:
            # reward | action | stream id (4 bytes each) | done | truncated (1 each), packed for the row count in use
            mk = lambda nbytes: (torch.zeros(nbytes, dtype=torch.uint8, pin_memory=True),
                                 torch.zeros(nbytes, dtype=torch.uint8, device=self.device))
            with torch.cuda.device(self.device):
                self._ing = _Staging(lambda: dict(rows=rows, views={}, obs=mk(4 * rows * O), next=mk(4 * rows * O),
                                                  small=mk(14 * rows)))
        st = self._ing.acquire()
        v = st["views"].get((n, kind))
        if v is None:
            ob, odt = (4 * n * O, torch.float32) if kind == N.OBS_F32 else (n * O, torch.uint8)
            small = lambda t: dict(reward=t[0:4 * n].view(torch.float32), action=t[4 * n:8 * n].view(torch.int32),
                                   ids=t[8 * n:12 * n].view(torch.int32), done=t[12 * n:13 * n], trunc=t[13 * n:14 * n])
            h, d = small(st["small"][0]), small(st["small"][1])
            for k in ("obs", "next"):
                h[k], d[k] = (t[:ob].view(odt).view(n, O) for t in st[k])
            v = {k: (h[k].numpy(), d[k]) for k in h}
            v["copies"] = dict(obs=(d["obs"], h["obs"]), next=(d["next"], h["next"]),
                               small=(st["small"][1][:14 * n], st["small"][0][:14 * n]))
            if len(st["views"]) >= 8:                  # (a collector that varies its subset size: keep the cache small)
                st["views"].clear()
            st["views"][(n, kind)] = v
        return v

    def extend_batch(self, obs, next_obs, action, reward, done, truncated, stream_ids=None):
        """One step of a vectorised collector: row i is the transition (obs[i], action[i], reward[i], next_obs[i],
        done[i], truncated[i]) of environment stream ``stream_ids[i]`` (None: stream i).  Equal, bit for bit, to the same
        transitions handed to ``extend()`` as linked ``Timestep`` chains -- one kernel launch, no per-row host work:
        predecessors come from a device table of each stream's open row.  Stream ids within one call must be distinct.

        NumPy arrays / host tensors travel through pinned staging; device tensors are used in place and nothing
        synchronises (a repeated id in a DEVICE id array cannot be refused here: its rows are stored unlinked and
        ``check_status()`` raises; nor can the table grow for them: device-side ids must lie below the table's size, 64 or
        what ``reserve_streams()`` / earlier calls made it).  ``obs`` / ``next_obs`` may be float32 or bool / uint8 (widened
        on the device), both of the same class.
        A stream's row links back to the stream's previous row while the episode goes on (not done, not truncated);
        ``next_obs`` is kept as the successor observation when truncated or not done.  Returns the first slot.

        With ``reward_clipping_type="dopamine_clamp"`` the stored reward is clamped to [-1, 1] on the device (``extend()``
        never clips: its caller, the reference's collector, already has); after ``track_episodes()`` the same launch keeps
        the episode returns.  Neither changes anything else the call writes."""
        if self.reward_clipping_type == "sign":
            raise ValueError('extend_batch: reward_clipping_type "sign" is r / abs(r) in the reference '
                             "(collector_process_interface.py:137), a division by zero at the first zero reward; it is not "
                             "reproduced here")
        if not torch.is_tensor(obs):
            obs = np.asarray(obs)
        n = int(obs.shape[0])
        if not 1 <= n <= self.capacity:
            raise ValueError(f"extend_batch: n = {n} rows must be in [1, capacity = {self.capacity}]")
        if not torch.is_tensor(next_obs):
            next_obs = np.asarray(next_obs)
        kind = _obs_kind(obs, next_obs)
        if self._ring_kind and kind == N.OBS_F32:
            # floats into a byte ring: what the host can see is checked here (and, where both arrays are the host's, sent
            # as the bytes themselves); a device tensor is narrowed by the kernel, which can only raise the status bit
            on_host = [not _is_dev(x) for x in (obs, next_obs)]
            as_bytes = [_narrow_host(_host(x), "extend_batch") if h else x for x, h in zip((obs, next_obs), on_host)]
            if all(on_host):
                (obs, next_obs), kind = as_bytes, N.OBS_U8
        ids_host, need = _check_stream_ids(stream_ids, n, 0 if self._stream_tab is None else self._stream_tab.numel())
        if self._desc is None:
            self._allocate(tuple(obs.shape[1:]))
        self.flush()                                   # rows staged by extend() come first
        O, odt = self.obs_elems, torch.float32 if kind == N.OBS_F32 else torch.uint8
        rows = [("obs", obs, (n, O), odt), ("next", next_obs, (n, O), odt), ("reward", reward, n, torch.float32),
                ("action", action, n, torch.int32), ("done", done, n, torch.uint8), ("trunc", truncated, n, torch.uint8)]
        if stream_ids is not None:
            rows.append(("ids", stream_ids if ids_host is None else ids_host, n, torch.int32))
        tab = self._stream_table(need)
        staged = not all(_is_dev(r[1]) for r in rows)
        v = self._ingest_views(n, kind) if staged else {}
        dev, copies = {"ids": None}, {}
        for k, x, shape, dtype in rows:
            dev[k], was_staged = _device_array(x, shape, dtype, v.get(k))
            if was_staged:                             # (at most three copies: obs, next, the scalar block whole)
                copies[k if k in ("obs", "next") else "small"] = True
        for k in copies:
            v["copies"][k][0].copy_(v["copies"][k][1], non_blocking=True)
        w, smp = self.buffer._writer, self.buffer._sampler
        first, serial = w._cursor, self._serial
        # neither a clamp nor tracking: the entry point, arguments and launch of before; either: the same launch with one
        # more workgroup (and the clip), the episode descriptor behind the arguments
        name, tail = "prism_replay_ingest", ()
        if self._ep is not None or self._clip != N.CLIP_NONE:
            if self._ep_desc is None:
                self._bind_episode_desc()
            name, tail = "prism_replay_ingest_tracked", (self._ep_desc_ref,)
        head = ()
        if self._ring_kind:                            # one entry point for both launches: the descriptor, or NULL
            name, head, tail = "prism_replay_ingest_ring", (self._ring_kind,), tail or (None,)
        self._call(name, *head, n, first, serial, N.ptr(dev["obs"]), N.ptr(dev["next"]), kind,
                   N.ptr(dev["reward"]), N.ptr(dev["action"]), N.ptr(dev["done"]), N.ptr(dev["trunc"]), N.ptr(dev["ids"]),
                   N.ptr(tab), tab.numel(), smp._alpha, smp._eps, *tail, submit=self._ing if staged else None)
        return self._mirror_rows(n)                    # host mirrors, by arithmetic

    # ------------------------------------------------------------------ the cursor form: a launch a hipGraph can replay
    def seed_cursor(self, slot):
        """Before a launch (or a replay whose first launch) reads ``cursor[slot]``: make the word hold the host's count.  A
        store on the stream, and only when an eager ingest, a bulk load, a restore -- or a caller that picks another slot --
        has moved the count since the last cursor launch (the rule ``HipAgent._forward_graph`` follows for its counters)."""
        if self._cursor_words is None:
            self._cursor_words = torch.zeros(2, dtype=torch.int64, device=self.device)
        if self._cursor_known != (slot, self._serial):
            self._cursor_words[slot] = self._serial
            self._cursor_known = (slot, self._serial)

    def enqueue_extend_cursor(self, slot, obs, next_obs, action, reward, done, truncated):
        """``extend_batch`` as ONE launch that takes the ring cursor from ``cursor[slot]`` on the device and leaves the
        advanced count in ``cursor[slot ^ 1]`` (``prism_replay_ingest_cursor``): enqueue only, safe inside a stream capture.
        Device tensors only, used in place (observations float32 or uint8, ``action`` int32, ``reward`` float32, ``done`` /
        ``truncated`` uint8, all contiguous), row i is stream i; the ring, the stream table and (when tracking) the episode
        arrays must already be there and sized -- nothing is allocated, staged or converted here, and no host mirror moves
        (``extend_cursor_mirror`` does that, once per launch that ran)."""
        n = int(obs.shape[0])
        if self._desc is None or self._stream_tab is None or self._stream_tab.numel() < n or self._cursor_words is None:
            raise RuntimeError("enqueue_extend_cursor: the ring, a stream table of n entries and the cursor words (seed_cursor) "
                               "must exist before the launch is enqueued")
        if slot not in (0, 1) or not 1 <= n <= self.capacity:
            raise ValueError("enqueue_extend_cursor: slot must be 0 or 1 and n in [1, capacity]")
        if self._n_staged:
            raise RuntimeError("enqueue_extend_cursor: rows staged by extend() come first (flush())")
        if self.reward_clipping_type == "sign":
            raise ValueError('enqueue_extend_cursor: reward_clipping_type "sign" is not reproduced (see extend_batch)')
        want = dict(obs=(torch.float32, torch.uint8), next_obs=(obs.dtype,), action=(torch.int32,), reward=(torch.float32,),
                    done=(torch.uint8,), truncated=(torch.uint8,))
        given = dict(obs=obs, next_obs=next_obs, action=action, reward=reward, done=done, truncated=truncated)
        for k, x in given.items():
            rows = n * self.obs_elems if k in ("obs", "next_obs") else n
            if not (_is_dev(x) and x.dtype in want[k] and x.is_contiguous() and x.numel() == rows):
                raise ValueError(f"enqueue_extend_cursor: {k} must be a contiguous device tensor of {rows} elements, dtype "
                                 f"{' / '.join(str(t) for t in want[k])}")
        ep = None
        if self._ep is not None or self._clip != N.CLIP_NONE:
            if self._ep_desc is None:
                self._bind_episode_desc()
            ep = self._ep_desc_ref
        smp, tab = self.buffer._sampler, self._stream_tab
        self._call("prism_replay_ingest_cursor", self._ring_kind, n, N.ptr(self._cursor_words), slot, N.ptr(obs),
                   N.ptr(next_obs), N.OBS_F32 if obs.dtype == torch.float32 else N.OBS_U8, N.ptr(reward), N.ptr(action),
                   N.ptr(done), N.ptr(truncated), None, N.ptr(tab), tab.numel(), smp._alpha, smp._eps, ep)

    def extend_cursor_mirror(self, n, slot):
        """The host mirrors of one cursor launch of ``n`` rows that read ``cursor[slot]``, by ``extend_batch``'s arithmetic."""
        first = self._mirror_rows(n)
        self._cursor_known = (slot ^ 1, self._serial)
        return first

    def _mirror_rows(self, n):
        """``n`` rows went into the ring behind the writer: cursor, serial, size, and the slots' ids from a private
        (negative) range -- no Timestep id matches them.  Returns the first slot."""
        w, cap, serial = self.buffer._writer, self.capacity, self._serial
        first = w._cursor
        own = np.arange(-2 - serial, -2 - serial - n, -1, dtype=np.int64)
        head = min(n, cap - first)
        self._slot_id[first:first + head] = own[:head]
        self._slot_id[:n - head] = own[head:]
        w._cursor = (first + n) % cap
        self._serial = serial + n
        self._size = min(self._size + n, cap)
        return first

    @torch.no_grad()
    def sample(self, batch_size=None, return_info=False):
        if self._size == 0 and self._n_staged == 0:
            raise RuntimeError("Cannot sample from an empty storage.")
        self.flush()
        B = self.buffer._batch_size if batch_size is None else int(batch_size)
        offset = self._draws + self._fused_draws
        self._batch_for(B)
        if self.use_per:
            mass = None
            if self.mass_rng == "numpy":
                self._call("prism_per_query", self._size, N.ptr(self._q2))
                p_sum, p_min = self._q2.tolist()
                if p_sum <= 0 or p_min <= 0:
                    raise RuntimeError("non-positive p_sum / p_min")
                m = np.random.uniform(0.0, p_sum, size=B).astype(np.float32)
                self._mass.copy_(torch.from_numpy(m))
                mass = self._mass
            self._call("prism_per_sample", self._size, B, N.ptr(mass), self.seed, offset, self.buffer._sampler._beta,
                       N.ptr(self._index), N.ptr(self._weight))
        else:
            self._call("prism_uniform_sample", self._size, B, self.seed, offset, N.ptr(self._index), desc=False)
        self._draws += B
        self._gather_into_batch(B)
        if self.strict:
            self.check_status()
        if return_info:
            info = {"index": self._index}
            if self.use_per:
                info["_weight"] = self._weight
            return self._batch, info
        return self._batch

    def _batch_for(self, B):
        """The index array of the static batch, (re)allocated for B rows."""
        if self._index is None or self._index.shape[0] != B:
            self._alloc_batch(B)
        return self._index

    def _gather_into_batch(self, B):
        """n-step walk + row gather of the slots in ``_index`` into the static batch."""
        name, head = ("prism_replay_gather_ring", (self._ring_kind,)) if self._ring_kind else ("prism_replay_gather", ())
        self._call(name, *head, N.ptr(self._index), B, N.ptr(self._obs), N.ptr(self._next_obs),
                   N.ptr(self._reward), N.ptr(self._nonterminal), N.ptr(self._gamma), N.ptr(self._action))

    @torch.no_grad()
    def gather(self, indices):
        """The static batch for given slots: n-step return + collate (timestep_buffer.py:79-238) without sampling."""
        self.flush()
        idx = torch.as_tensor(indices).to(self.device, torch.int64).reshape(-1).contiguous()
        B = int(idx.numel())
        self._batch_for(B).copy_(idx)
        self._gather_into_batch(B)
        return self._batch

    def check_status(self):
        """Raise what torchrl would have raised at sample time (costs one D2H sync)."""
        bits = int(self.status.item())
        if bits & (N.STATUS_NONPOSITIVE_PSUM | N.STATUS_NONPOSITIVE_PMIN):
            raise RuntimeError("non-positive p_sum / p_min in the priority trees")
        if bits & N.STATUS_INGEST_DUP_STREAM:
            raise RuntimeError("extend_batch: a device-side stream_ids array held a repeated or out-of-range id "
                               "(its rows were stored unlinked)")
        if bits & N.STATUS_OBS_INEXACT:
            raise RuntimeError("extend_batch: a device-side float observation was not byte-exact (+0.0, 1.0 .. 255.0); "
                               "obs_storage='uint8' stored it as 0")
        if bits & N.STATUS_INGEST_BAD_CURSOR:
            raise RuntimeError("enqueue_extend_cursor: a launch read a negative ring cursor from the device (it wrote nothing "
                               "to the ring)")
        if bits & N.STATUS_FRONT_BAD_SIZE:
            raise RuntimeError("prism_step_front_cursor: a launch read a ring size <= 0 from the device cursor (it sampled "
                               "as from a ring of one row)")

    def update_priority(self, indices, priorities, take_abs=False):
        if not self.use_per:
            return
        idx = torch.as_tensor(indices).to(self.device, torch.int64).reshape(-1).contiguous()
        pr = torch.as_tensor(priorities).detach().to(self.device, torch.float32).reshape(-1)
        if pr.numel() == 1 and idx.numel() > 1:
            pr = pr.expand(idx.numel())
        smp = self.buffer._sampler
        self._call("prism_per_update", N.ptr(idx), N.ptr(pr.contiguous()), idx.numel(), smp._alpha, smp._eps, int(take_abs))

    def set_static_batch(self, batch):
        self._batch = batch
        self._obs = batch["observation"]
        self._next_obs = batch["next"]["observation"]
        self._reward = batch["next"]["reward"]
        self._nonterminal = batch["nonterminal"]
        self._gamma = batch["gamma"]
        self._action = batch["action"]

    def get_static_batch(self):
        return self._batch

    def empty(self):
        if self._desc is not None:
            self._call("prism_replay_init")
        self._seal(0)

    # ------------------------------------------------------------------ bulk installs (bench / restore)
    def _seal(self, n, n_sampleable=None, cursor=None, leaves=None, back=None, slot_ids=None):
        """Step c of every bulk install -- after a. ``_allocate`` (an empty ring) and b. the caller's writes of rows [0, n)
        of ``obs`` .. ``link``: everything the ring's contents imply, set in ONE place.  The first ``n_sampleable`` rows are
        stored items (sampled, counted by len()), the rest only serve as link targets; the writer goes on at ``cursor``
        (default: behind the items).  ``leaves``: the items' tree leaves, [ns] or [ns, 2] as {sum, min} (default 1);
        ``back``: the inverse of ``link`` if the caller holds it (else derived); ``slot_ids``: the rows' Timestep ids
        (default 0 .. n - 1).  No stream has an open row (or an open tracked episode), no Timestep a pending predecessor, nothing
        is staged."""
        ns = n if n_sampleable is None else int(n_sampleable)
        self._size = ns
        self.buffer._writer._cursor = ns % self.capacity if cursor is None else int(cursor)
        self._serial = self.buffer._writer._cursor       # serial % capacity == writer cursor
        if self._stream_tab is not None:
            self._stream_tab.fill_(-1)
        self._close_episodes()
        self._slot_id[:] = -1
        self._slot_id[:n] = np.arange(n) if slot_ids is None else slot_ids
        self._pending.clear()
        self._n_staged = 0
        if n == 0:                                       # (empty(): prism_replay_init has left nothing to finish)
            return
        if back is None:
            lk = self.link[:n]
            valid = lk >= 0
            self.back[lk[valid].long()] = torch.arange(n, device=self.device, dtype=torch.int32)[valid]
        else:
            self.back[:n].copy_(back)
        if self.use_per:
            tc = self.tree_capacity
            p = torch.ones(ns, device=self.device) if leaves is None else torch.as_tensor(leaves)[:ns]
            self.tree[tc:tc + ns].copy_(p if p.dim() == 2 else p.unsqueeze(1))
            self._call("prism_per_rebuild")

    def _ring_rows(self, what, *arrays):
        """Observation arrays (host or device, bool / uint8 or floating point) as tensors a bulk install copies into the ring.
        A byte ring takes small-int arrays as they are and floats narrowed, after ONE reduction over all of them (one sync):
        a value that is not byte-exact is a ValueError, raised before the caller has touched the ring."""
        ts = [torch.as_tensor(x) for x in arrays]
        if not self._ring_kind:
            return ts
        out, ok = [], None
        for t in ts:
            if t.dtype in _SMALL_INT[True]:
                out.append(t.to(torch.uint8))
                continue
            t = t.to(torch.float32)
            e = _byte_exact(t).to(self.device)
            ok = e if ok is None else ok & e
            out.append(_as_u8(t))
        if ok is not None and not bool(ok.item()):
            raise ValueError(f"{what}: obs_storage='uint8' holds only byte-exact observations (+0.0, 1.0 .. 255.0); "
                             "nothing was written")
        return out

    def load_arrays(self, obs, succ_obs, reward, action, flags, link, priorities=None, n_sampleable=None, cursor=None,
                    slot_ids=None):
        """Replace the buffer's contents by n rows from device/host arrays, with the trees rebuilt from the given leaf
        values (already (p+eps)**alpha).  Used for synthetic pre-fill and restore.  ``n_sampleable`` < n: only the
        first rows are stored items (sampled, counted by len()); the rest only serve as link targets.  ``cursor`` /
        ``slot_ids``: where the writer goes on and the rows' Timestep ids, when a saved directory holds them (``_seal``).
        Nothing of what the buffer held before survives: the result is that of loading into a fresh buffer."""
        n = int(obs.shape[0])
        obs, succ_obs = self._ring_rows("load_arrays", obs, succ_obs)
        self._allocate(tuple(obs.shape[1:]))
        O = self.obs_elems
        self.obs[:n].copy_(obs.reshape(n, O))
        self.succ_obs[:n].copy_(succ_obs.reshape(n, O))
        self.reward[:n].copy_(torch.as_tensor(reward))
        self.action[:n].copy_(torch.as_tensor(action))
        self.flags[:n].copy_(torch.as_tensor(flags))
        self.link[:n].copy_(torch.as_tensor(link).to(self.device, torch.int32))
        self._seal(n, n_sampleable, cursor, priorities, slot_ids=slot_ids)

    def save(self, path):
        """``TimestepBuffer.save`` (timestep_buffer.py:259-296): ``experience_buffer/timesteps.pkl`` in the reference's
        format (ref_format.py).  The reference also writes torchrl's sampler / writer dumps there -- third-party formats
        that cannot be pinned; priorities, running maximum and the ring cursor go to ``hip_sampler.pt``."""
        from prism_amd.experience import ref_format
        self.flush()
        d = os.path.join(path, "experience_buffer")
        os.makedirs(d, exist_ok=True)
        n = self._size
        # (a byte ring widens: the file is byte for byte what the fp32 ring holding the same rows writes)
        flat = ref_format.serialize_ring(self.obs[:n].cpu().float().numpy(), self.succ_obs[:n].cpu().float().numpy(),
                                         self.reward[:n].cpu().numpy(), self.action[:n].cpu().numpy(),
                                         self.flags[:n].cpu().numpy(), self.link[:n].cpu().numpy(),
                                         self.back[:n].cpu().numpy(), self._slot_id[:n], self._obs_shape)
        with open(os.path.join(d, "timesteps.pkl"), "wb") as f:
            pickle.dump(flat, f)
        state = dict(size=n, cursor=self.buffer._writer._cursor, per_state=self.per_state.cpu())
        if self.use_per:
            tc = self.tree_capacity
            state["leaves"] = self.sum_tree[tc:tc + n].cpu()
        torch.save(state, os.path.join(d, "hip_sampler.pt"))

    def load(self, path):
        """``TimestepBuffer.load`` (timestep_buffer.py:298-318) of a file written here or by the reference; without
        ``hip_sampler.pt`` (a reference-written directory) every slot starts at the default priority."""
        from prism_amd.experience import ref_format
        d = os.path.join(path, "experience_buffer")
        from prism_amd.util import ref_pickle
        with open(os.path.join(d, "timesteps.pkl"), "rb") as f:
            flat = ref_pickle.load_plain(f)        # a flat list of numbers and booleans: no class may be named
        r = ref_format.ring_from_timesteps(flat)
        n, n_all = int(r["n_kept"]), min(int(r["obs"].shape[0]), self.capacity)
        if n > self.capacity:
            raise ValueError(f"the file holds {n} complete timesteps, this buffer only {self.capacity} "
                             "(experience_replay_capacity): load it into a buffer at least as large")
        sp = os.path.join(d, "hip_sampler.pt")
        st = torch.load(sp, weights_only=True) if os.path.exists(sp) else None
        leaves = None
        if st is not None and "leaves" in st and int(st["size"]) == n:
            leaves = st["leaves"]
        elif self.use_per:
            smp = self.buffer._sampler
            leaves = torch.full((n,), float(np.float32(np.float32(1.0 + smp._eps) ** np.float32(smp._alpha))))
        link = np.where(r["link"][:n_all] < n_all, r["link"][:n_all], -1)
        self.load_arrays(r["obs"][:n_all], r["succ_obs"][:n_all], r["reward"][:n_all], r["action"][:n_all], r["flags"][:n_all],
                         link, leaves, n_sampleable=n, cursor=None if st is None else int(st["cursor"]),
                         slot_ids=r["ids"][:n_all])
        if st is not None:
            self.per_state.copy_(st["per_state"])

    # ------------------------------------------------------------------ exact resume (prism_amd/util/snapshot.py)
    def _compat_record(self):
        """What a snapshot must share with the buffer it is loaded into."""
        return dict(capacity=self.capacity, obs_shape=None if self._obs_shape is None else list(self._obs_shape),
                    n_step=self.n_step, gammas=[float(g) for g in self.gammas], use_per=self.use_per,
                    mass_rng=str(self.mass_rng))

    def _valid_rows(self):
        """Rows of the ring arrays that hold anything: all of them once the ring has wrapped, else up to the highest row ever
        written (link-target rows a reference-format load() placed behind ``_size`` included)."""
        if self._size >= self.capacity:
            return self.capacity
        used = np.flatnonzero(self._slot_id != -1)
        return max(self._size, int(used[-1]) + 1 if used.size else 0)

    def _state_part(self):
        """Part ``replay`` of a snapshot: the live ring, its host mirrors and counters, as plain data."""
        self.flush()
        if self._desc is None:
            raise RuntimeError("save_state: the buffer holds nothing yet (no observation shape)")
        self.check_status()
        rows, n = self._valid_rows(), self._size
        obs, succ = self.obs[:rows], self.succ_obs[:rows]
        # exact as uint8? compared in bit space (-0.0 is not 0), both arrays in one reduction, one D2H sync
        # (a byte ring is that by construction: no scan)
        small = rows > 0 and (bool(self._ring_kind) or bool((_byte_exact(obs) & _byte_exact(succ)).item()))
        pack = (lambda x: _as_u8(x).cpu()) if small and not self._ring_kind else (lambda x: x.cpu())
        smp = self.buffer._sampler
        part = dict(rows=rows, size=n, obs_shape=list(self._obs_shape), cursor=int(self.buffer._writer._cursor),
                    serial=int(self._serial),
                    obs_dtype="uint8" if small else "float32", obs=pack(obs), succ_obs=pack(succ),
                    reward=self.reward[:rows].cpu(), action=self.action[:rows].cpu(), flags=self.flags[:rows].cpu(),
                    link=self.link[:rows].cpu(), back=self.back[:rows].cpu(), per_state=self.per_state.cpu(),
                    slot_id=torch.from_numpy(self._slot_id[:rows].copy()),
                    pending=[[int(k), int(v[0]), int(v[1])] for k, v in self._pending.items()],
                    stream_tab=None if self._stream_tab is None else self._stream_tab.cpu(),
                    seed=int(self.seed), draws=int(self._draws + self._fused_draws),
                    alpha=float(smp._alpha), beta=float(smp._beta), eps=float(smp._eps))
        if self.use_per:
            tc = self.tree_capacity
            part["leaves"] = self.tree[tc:tc + n].cpu()          # {sum, min} of every stored item; the nodes above follow
        if self._ep is not None:                                 # (tracking off: the part is what it was without it)
            part["episodes"] = dict(ep_return=self._ep_return.cpu(), ep_length=self._ep_length.cpu(),
                                    stats=self._ep_stats.cpu(), counts=self._ep_counts.cpu(), ema=float(self._ep["ema"]),
                                    count_first_step=bool(self._ep["count_first_step"]))
        return part

    def _restore_part(self, part, keep_streams=True):
        rows, dev = int(part["rows"]), self.device
        # (a byte ring refuses an fp32 snapshot that holds a value it cannot store -- here, before anything is touched)
        src = dict(zip(("obs", "succ_obs"), self._ring_rows("load_state", part["obs"], part["succ_obs"])))
        self._allocate(tuple(int(s) for s in part["obs_shape"]))
        O = self.obs_elems
        for name in ("obs", "succ_obs"):
            getattr(self, name)[:rows].copy_(src[name].to(dev).reshape(rows, O))           # (uint8 into fp32 widens here)
        for name in ("reward", "action", "flags", "link"):
            getattr(self, name)[:rows].copy_(part[name].to(dev))
        self._seal(rows, part["size"], part["cursor"], part.get("leaves"), part["back"].to(dev), part["slot_id"].numpy())
        # what only a snapshot has, layered on the sealed ring: the sampler's state and counters ...
        self.per_state.copy_(part["per_state"].to(dev))
        self.seed = int(part["seed"])
        # one counter space for sample() and the fused step: a new agent's device word starts at 0, the sum is what counts
        self._draws, self._fused_draws = int(part["draws"]), 0
        smp = self.buffer._sampler
        smp._alpha, smp._beta, smp._eps = float(part["alpha"]), float(part["beta"]), float(part["eps"])
        # ... a stream table of the size the run had reached, and (keep_streams) the chains that were open in it
        tab = part["stream_tab"]
        self._stream_tab = None if tab is None else tab.to(dev, torch.int64).contiguous()
        if keep_streams:
            self._serial = int(part["serial"])
            self._pending = {int(k): (int(s), int(i)) for k, s, i in part["pending"]}
        elif tab is not None:
            self._stream_tab.fill_(-1)
        # ... and the episode bookkeeping: a snapshot that holds it turns tracking on as the run had it, one without it
        # leaves tracking as this buffer has it (open episodes closed by the seal above)
        eps = part.get("episodes")
        if eps is not None:
            self._ep = None
            self.track_episodes(eps["ema"], eps["count_first_step"])
            self._ep_return = eps["ep_return"].to(dev, torch.float64).contiguous()
            self._ep_length = eps["ep_length"].to(dev, torch.int32).contiguous()
            self._ep_stats.copy_(eps["stats"])
            self._ep_counts.copy_(eps["counts"])
            if not keep_streams:
                self._close_episodes()
        if self._ep is not None:
            if self._stream_tab is None:
                self._stream_table(1)
            self._fit_episode_arrays()

    def save_state(self, path):
        """The live ring as an exact-resume snapshot (part ``replay``): every row, link and tree leaf, the host mirrors, the
        open chains (``_pending``, the stream table) and the draw count -- what ``save()`` (the reference's format) cannot
        hold.  Observations travel as uint8 when every value is an integer in [0, 255] (bit-exact either way)."""
        from prism_amd.util import snapshot
        part = self._state_part()
        return snapshot.write_snapshot(path, {"replay": part}, {"compat": {"replay": self._compat_record()}})

    def _check_snapshot(self, manifest):
        from prism_amd.util import snapshot
        cur = self._compat_record()
        if cur["obs_shape"] is None:
            del cur["obs_shape"]
        snapshot.check_compat((manifest.get("compat") or {}).get("replay"), cur, "HipReplayBuffer.load_state")

    def load_state(self, path, keep_streams=True):
        """Restore a ``save_state`` snapshot into a freshly constructed buffer of the same configuration: what follows is
        bit-identical to the run that wrote it.  ``keep_streams=False`` closes every open chain (a collector that restarts
        its environments): the first row of every stream is then stored unlinked.  A snapshot of another capacity,
        observation shape, ``n_step``, gammas, ``use_per`` or ``mass_rng`` is refused before anything is touched.  ``obs_storage``
        is not part of that record: snapshots interchange between the two kinds whenever the observations are byte-exact
        (a uint8 ring refuses any other, also before anything is touched)."""
        from prism_amd.util import snapshot
        self._check_snapshot(snapshot.read_manifest(path))
        parts, _ = snapshot.read_snapshot(path, ["replay"])
        self._restore_part(parts["replay"], keep_streams)
