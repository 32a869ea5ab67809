"""``DeviceBreakout`` -- MinAtar Breakout for N lock-stepped environments, stepped by one launch of
``prism_env_breakout_step`` (include/prism_hip.h; the rules are DESIGN.md 7.3: a restatement of MinAtar v1 that is NOT
checked against the ``minatar`` package).  It is the ``VectorCollector`` protocol (prism_amd/collectors.py), so acting, the
environment step, the replay ingestion and the learner step sit on one stream and no host code reads an observation, a
reward or an episode end.

What ``step`` returns are views of persistent device buffers; nothing synchronises.

* ``reward`` / ``done`` / ``truncated`` / ``next_obs`` are valid until the next ``step`` on the same stream.
* The observation to act on alternates between two addresses: ``step`` writes the one ``observe()`` did NOT return last and
  leaves the other untouched, so the observation a step acted on can still be handed to ``extend_batch`` after it, and
  ``Agent.forward``'s captured launch reads either address in place (its "ptr" mode keeps one capture per address).
"""
import ctypes

import numpy as np
import torch

from prism_amd import _native as N
from prism_amd.experience.hip_replay import _Staging, _is_dev

OBS_SHAPE = (10, 10, 4)
_OBS_DTYPES = {"float32": (N.OBS_F32, torch.float32), "uint8": (N.OBS_U8, torch.uint8)}
_FIELDS = ("pos", "ball_x", "ball_y", "ball_dir", "last_x", "last_y", "strike", "last_action")
_SHIFTS = dict(pos=(0, 15), ball_x=(4, 15), ball_y=(8, 15), ball_dir=(12, 3), last_x=(16, 15), last_y=(20, 15), strike=(24, 1),
               last_action=(25, 7))
_NP = {torch.uint8: np.uint8, torch.float64: np.float64}
_LIMITS = dict(pos=9, ball_x=9, ball_y=9, ball_dir=3, last_x=9, last_y=9, strike=1, last_action=5)


def pack_state(fields):
    """The device's state block, int32 [N, 8], from a dict of host arrays: the small fields of ``_FIELDS`` [N], ``bricks``
    [N, 10, 10] (rows 1..3 only), ``ep_steps`` [N], ``t`` [N] (Python ints / uint64)."""
    n = len(fields["pos"])
    words = np.zeros((n, N.ENV_STATE_WORDS), np.uint32)
    bricks = np.asarray(fields["bricks"]).reshape(n, 10, 10) != 0
    if bricks[:, 0].any() or bricks[:, 4:].any():
        raise ValueError("DeviceBreakout.set_state: bricks outside rows 1..3")
    bits = bricks[:, 1:4].reshape(n, 30).astype(np.uint64)
    words[:, 0] = (bits << np.arange(30, dtype=np.uint64)).sum(axis=1).astype(np.uint32)
    for name in _FIELDS:
        v = np.asarray(fields[name]).astype(np.int64).reshape(n)
        if v.min() < 0 or v.max() > _LIMITS[name]:
            raise ValueError(f"DeviceBreakout.set_state: {name} outside [0, {_LIMITS[name]}]")
        words[:, 1] |= (v << _SHIFTS[name][0]).astype(np.uint32)
    words[:, 2] = np.asarray(fields["ep_steps"]).astype(np.uint32)
    t = np.array([int(x) for x in fields["t"]], dtype=np.uint64)
    words[:, 4], words[:, 5] = (t & np.uint64(0xFFFFFFFF)).astype(np.uint32), (t >> np.uint64(32)).astype(np.uint32)
    return words.view(np.int32)


def unpack_state(words):
    """The inverse of ``pack_state``: a dict of host arrays (``t`` as uint64)."""
    w = np.ascontiguousarray(words).view(np.uint32).reshape(-1, N.ENV_STATE_WORDS)
    n = w.shape[0]
    out = {name: ((w[:, 1] >> sh) & mask).astype(np.int32) for name, (sh, mask) in _SHIFTS.items()}
    bricks = np.zeros((n, 10, 10), np.uint8)
    bricks[:, 1:4] = ((w[:, 0:1] >> np.arange(30, dtype=np.uint32)) & 1).astype(np.uint8).reshape(n, 3, 10)
    out["bricks"] = bricks
    out["ep_steps"] = w[:, 2].astype(np.int64)
    out["t"] = w[:, 4].astype(np.uint64) | (w[:, 5].astype(np.uint64) << np.uint64(32))
    return out


class DeviceBreakout:
    def __init__(self, n_envs, seed, device="cuda:0", sticky_action_prob=0.0, episode_timestep_limit=0, minimal_actions=False,
                 obs_dtype="float32"):
        n_envs, limit, p = int(n_envs), int(episode_timestep_limit or 0), float(sticky_action_prob)
        if not 1 <= n_envs <= N.ENV_MAX:
            raise ValueError(f"DeviceBreakout: n_envs must be in [1, {N.ENV_MAX}]")
        if not 0.0 <= p <= 1.0:
            raise ValueError("DeviceBreakout: sticky_action_prob must be in [0, 1]")
        if limit < 0 or limit >= 2 ** 31:
            raise ValueError("DeviceBreakout: episode_timestep_limit must be in [0, 2^31)")
        if obs_dtype not in _OBS_DTYPES:
            raise ValueError(f"DeviceBreakout: obs_dtype = {obs_dtype!r} must be one of {sorted(_OBS_DTYPES)}")
        if not str(device).startswith("cuda"):
            raise N.NativeLibraryError("DeviceBreakout needs a GPU device; there is no CPU fallback")
        N.lib()
        self.n_envs, self.seed, self.device = n_envs, int(seed) & (2 ** 64 - 1), torch.device(device)
        self.sticky_action_prob, self.episode_timestep_limit, self.minimal_actions = p, limit, bool(minimal_actions)
        self.obs_dtype = obs_dtype
        self.n_actions, self.obs_shape = (3 if minimal_actions else 6), OBS_SHAPE
        kind, dtype = _OBS_DTYPES[obs_dtype]
        self._on_device = torch.cuda.device(self.device)
        dev = self.device
        with self._on_device:
            self._state = torch.zeros((n_envs, N.ENV_STATE_WORDS), dtype=torch.int32, device=dev)
            self._status = torch.zeros(1, dtype=torch.int32, device=dev)
            self._obs = torch.zeros((2, n_envs) + OBS_SHAPE, dtype=dtype, device=dev)
            self._next_obs = torch.zeros((n_envs,) + OBS_SHAPE, dtype=dtype, device=dev)
            self._reward = torch.zeros(n_envs, dtype=torch.float32, device=dev)
            self._done = torch.zeros(n_envs, dtype=torch.uint8, device=dev)
            self._truncated = torch.zeros(n_envs, dtype=torch.uint8, device=dev)
        d = N.EnvDesc()
        d.n_envs, d.n_actions, d.step_limit, d.obs_kind, d.sticky_p, d.seed = n_envs, self.n_actions, limit, kind, p, self.seed
        d.state, d.status = self._state.data_ptr(), self._status.data_ptr()
        d.obs[0], d.obs[1], d.next_obs = self._obs[0].data_ptr(), self._obs[1].data_ptr(), self._next_obs.data_ptr()
        d.reward, d.done, d.truncated = self._reward.data_ptr(), self._done.data_ptr(), self._truncated.data_ptr()
        self._desc, self._desc_ref = d, ctypes.byref(d)
        self._parity = 0               # the ping-pong buffer that holds the observation to act on
        self._started = False
        self._stage = None
        self.closed = False

    # ------------------------------------------------------------------ the VectorCollector protocol
    def reset(self, first_side=None):
        """Start every environment: a fresh first episode, lifetime step count 0.  ``first_side`` (tests): the sides, 0 / 1,
        in place of the draws."""
        with self._on_device:
            side = None if first_side is None else self._dev(first_side, torch.uint8)
            N.check(N.lib().prism_env_breakout_reset(self._desc_ref, N.ptr(side), N.current_stream_handle()),
                    "prism_env_breakout_reset")
        self._parity, self._started = 0, True
        return self._obs[0]

    def observe(self):
        """The observations to act on next (a fresh one where an episode ended): one of two persistent buffers."""
        self._need_started("observe")
        return self._obs[self._parity]

    def step(self, actions, u=None, side=None):
        """One step of every environment -> (next_obs, reward, done, truncated), views of persistent device buffers.
        ``actions``: a device int64 tensor is read in place; anything else goes through a pinned rotation.  ``u`` / ``side``
        (tests): the sticky coins (float64) and the sides of the episodes that begin, in place of the draws."""
        self._need_started("step")
        n = self.n_envs
        with self._on_device:
            staged = not (_is_dev(actions) and actions.dtype == torch.int64 and actions.is_contiguous())
            if staged and _is_dev(actions):
                act, staged = actions.to(torch.int64).contiguous(), False
            elif staged:
                act = self._stage_actions(actions)
            else:
                act = actions
            if act.numel() != n:
                raise ValueError(f"DeviceBreakout.step: {act.numel()} actions for {n} environments")
            u_dev = None if u is None else self._dev(u, torch.float64)
            side_dev = None if side is None else self._dev(side, torch.uint8)
            N.check(N.lib().prism_env_breakout_step(self._desc_ref, N.ptr(act), N.ptr(u_dev), N.ptr(side_dev), self._parity,
                                                    N.current_stream_handle()), "prism_env_breakout_step")
            if staged:
                self._stage.submit()
        self._parity ^= 1
        return self._next_obs, self._reward, self._done, self._truncated

    def close(self):
        """Drains the staging rotation and checks the device status word (one small device-to-host copy)."""
        if self.closed:
            return
        self.closed = True
        if self._stage is not None:
            self._stage.drain()
        self.check_status()

    def check_status(self):
        """Raise if a step has seen an action outside [0, n_actions) since the last check (it acted as no-op)."""
        status = int(self._status.item())
        if status & N.ENV_STATUS_BAD_ACTION:
            self._status.zero_()
            raise N.PrismError(f"DeviceBreakout: a step was given an action outside [0, {self.n_actions}); it acted as no-op")

    # ------------------------------------------------------------------ state, for tests and resume
    def get_state(self):
        """The state of every environment as a dict of host arrays (synchronises)."""
        return unpack_state(self._state.cpu().numpy())

    def set_state(self, fields):
        """Install a state (the dict ``get_state`` returns) and redraw the acting observation from it: afterwards
        ``observe()`` shows the installed state.  Synchronises; for tests and resume, not for the loop."""
        words = pack_state(fields)
        if words.shape[0] != self.n_envs:
            raise ValueError("DeviceBreakout.set_state: one state per environment")
        with self._on_device:
            self._state.copy_(torch.from_numpy(words))
            self._obs[0].copy_(torch.from_numpy(render(fields)).to(self._obs.dtype))
        self._parity, self._started = 0, True

    def state_dict(self):
        """Plain data for an exact-resume snapshot: the state block (the draws follow from it and the seed)."""
        return dict(kind="DeviceBreakout", n_envs=self.n_envs, n_actions=self.n_actions, seed=self.seed,
                    started=bool(self._started), state=self._state.cpu().clone())

    def load_state_dict(self, state):
        for name in ("kind", "n_envs", "n_actions", "seed"):
            have = "DeviceBreakout" if name == "kind" else getattr(self, name)
            if state[name] != have:
                raise ValueError(f"DeviceBreakout.load_state_dict: {name} = {state[name]!r} in the snapshot, {have!r} here")
        if state["started"]:
            self.set_state(unpack_state(state["state"].numpy()))
        else:
            self._started = False

    # ------------------------------------------------------------------
    def _need_started(self, what):
        if not self._started:
            raise RuntimeError(f"DeviceBreakout.{what}: call reset() first")

    def _dev(self, x, dtype):
        if _is_dev(x):
            x = x.to(dtype).contiguous()
        else:
            x = torch.from_numpy(np.ascontiguousarray(np.asarray(x).reshape(-1).astype(_NP[dtype]))).to(self.device)
        if x.numel() != self.n_envs:
            raise ValueError("DeviceBreakout: one value per environment")
        return x

    def _stage_actions(self, actions):
        """Host actions (NumPy array / host tensor / list) through a rotation of two pinned blocks, as ``EvalTracker``'s."""
        if self._stage is None:
            n = self.n_envs
            mk = lambda: (torch.zeros(n, dtype=torch.int64, pin_memory=True), torch.zeros(n, dtype=torch.int64, device=self.device))
            self._stage = _Staging(mk)
        host, dev = self._stage.acquire()
        a = actions.numpy() if torch.is_tensor(actions) else np.asarray(actions)
        np.copyto(host.numpy(), a.reshape(-1), casting="unsafe")
        dev.copy_(host, non_blocking=True)
        return dev


def render(fields):
    """The observation of a state dict, uint8 [N, 10, 10, 4]: paddle | ball | last ball cell | bricks.  Only ``set_state``
    draws an image on the host (there is no launch that only draws); every image of a run is the kernel's."""
    n = len(fields["pos"])
    img = np.zeros((n,) + OBS_SHAPE, np.uint8)
    i = np.arange(n)
    img[i, 9, np.asarray(fields["pos"]), 0] = 1
    img[i, np.asarray(fields["ball_y"]), np.asarray(fields["ball_x"]), 1] = 1
    img[i, np.asarray(fields["last_y"]), np.asarray(fields["last_x"]), 2] = 1
    img[..., 3] = np.asarray(fields["bricks"]).reshape(n, 10, 10) != 0
    return img
