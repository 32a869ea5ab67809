"""Evaluation: greedy runs over N environments stepped in lockstep, with the bookkeeping on the device.

``VectorEvaluator`` stands where the reference has ``SyncAgentEvaluator``
(``/root/reference/prism/evals/sync_agent_evaluator.py``) and ``CheckpointEvaluator`` where it has
``CheckpointAgentEvaluator`` (``checkpoint_agent_evaluator.py``): same surface, but the environments are the
``VectorCollector`` protocol (prism_amd/collectors.py: ``reset``, ``step``, ``observe``, ``n_actions``, ``obs_shape``) and the
episode returns, the list of finished episodes and the loop's stopping rule live in ``prism_eval_track``
(include/prism_hip.h): one launch per environment step, reward and done never read by the host.

An evaluation draws its quantile samples on the agent's acting stream at ``EVAL_DRAW_BASE`` + the evaluator's own running
count (``HipAgent.acting_stream``): the training draws are where they were when it ends, so a run with evaluations computes
what the run without them computes.
"""
import ctypes
import math
import os
import warnings

import numpy as np
import torch

from prism_amd import _native as N
from prism_amd.experience.hip_replay import _Staging, _device_array, _is_dev

EVAL_DRAW_BASE = 2 ** 62          # acting-stream counters of evaluations start here (the counters are 64-bit)
# Under the quota rule the host cannot count its way to the end, so it asks the device every this many steps.  A question
# is an event wait that drains the launches the host has run ahead by; a step costs the host 40-45 us of enqueue at small
# N, so one wait in 16 steps keeps the device fed, and at most 15 steps run behind the closing call (the tracker takes
# none of them) against the hundreds an evaluation lasts.  Fixed, not adaptive: the steps issued, and with them the acting
# draws an evaluation consumes, are then a function of the closing call alone, not of timing.
EVAL_QUOTA_POLL_STEPS = 16


class EvalTracker:
    """The device arrays of one evaluation over ``n_streams`` environments and the calls on them.  ``budget`` is the
    reference's ``evaluation_timestep_horizon``; the first ``log_capacity`` finished episodes are kept one by one, the
    sums, extremes and counts cover all of them.

    ``episodes_per_stream`` = E >= 1 switches to the quota rule (``prism_eval_track_quota``): every stream contributes
    exactly its first E finished episodes and the evaluation closes when every stream has, or after ``max_calls`` taken
    calls; ``budget`` is then not read by the device.  0 (the default) is the budget rule, the reference's."""

    def __init__(self, n_streams, budget, log_capacity=4096, device="cuda:0", episodes_per_stream=0, max_calls=0):
        n_streams, budget, log_capacity = int(n_streams), int(budget), int(log_capacity)
        episodes_per_stream, max_calls = int(episodes_per_stream), int(max_calls)
        if not 0 <= episodes_per_stream < 2 ** 31:
            raise ValueError("EvalTracker: episodes_per_stream must be >= 0")
        if episodes_per_stream and max_calls < 1:
            raise ValueError("EvalTracker: the quota rule needs max_calls >= 1 (the cap that closes an evaluation whose "
                             "streams do not all meet the quota)")
        if not 1 <= n_streams <= N.INGEST_MAX_STREAMS:
            raise ValueError(f"EvalTracker: n_streams must be in [1, {N.INGEST_MAX_STREAMS}]")
        if budget < 0 or not 0 <= log_capacity < 2 ** 31:
            raise ValueError("EvalTracker: budget and log_capacity must be >= 0")
        N.lib()
        self.n_streams, self.budget, self.log_capacity = n_streams, budget, log_capacity
        self.episodes_per_stream, self.max_calls = episodes_per_stream, max_calls
        self.device = torch.device(device)
        self._on_device = torch.cuda.device(self.device)
        cap = log_capacity
        with self._on_device:
            # stats (float64 [4]) | counts (int64 [4]) | log_return (float64 [cap]) | log_length (int32 [cap]) in ONE
            # block of 8-byte words: result() is one device-to-host copy
            # (under the quota rule qcounts (int64 [2]) follows the log in the same block)
            self._words = torch.zeros(8 + cap + (cap + 1) // 2 + (2 if episodes_per_stream else 0), dtype=torch.int64,
                                      device=self.device)
            self._ep_return = torch.zeros(n_streams, dtype=torch.float64, device=self.device)
            self._ep_length = torch.zeros(n_streams, dtype=torch.int32, device=self.device)
            self._host_counts = torch.zeros(2, dtype=torch.int64).pin_memory()
        w = self._words
        d = N.EvalDesc()
        d.n_streams, d.log_capacity, d.budget = n_streams, cap, budget
        d.ep_return, d.ep_length = self._ep_return.data_ptr(), self._ep_length.data_ptr()
        d.stats, d.counts = w.data_ptr(), w.data_ptr() + 32
        if cap:
            d.log_return, d.log_length = w.data_ptr() + 64, w.data_ptr() + 64 + 8 * cap
        d.host_counts = self._host_counts.data_ptr()
        self._desc, self._desc_ref = d, ctypes.byref(d)
        self._stage, self._views = None, {}
        self._quota = self._quota_ref = None
        if episodes_per_stream:
            with self._on_device:
                self._ep_done = torch.zeros(n_streams, dtype=torch.int32, device=self.device)
                self._host_closed = torch.zeros(1, dtype=torch.int64).pin_memory()
            q = N.EvalQuota()
            q.quota, q.max_calls = episodes_per_stream, max_calls
            q.ep_done, q.qcounts = self._ep_done.data_ptr(), w.data_ptr() + 8 * (w.numel() - 2)
            q.host_closed = self._host_closed.data_ptr()
            self._quota, self._quota_ref = q, ctypes.byref(q)

    def reset(self):
        """A new evaluation: every array back to zero (waits for what is in flight first: it may still write the pinned
        words)."""
        with self._on_device:
            torch.cuda.current_stream().synchronize()
            self._words.zero_()
            self._ep_return.zero_()
            self._ep_length.zero_()
            if self._quota is not None:
                self._ep_done.zero_()
        self._host_counts.zero_()
        if self._quota is not None:
            self._host_closed.zero_()

    def _staging(self, n):
        """The pinned set the next call fills (a ``_Staging`` rotation of two, guarded by events), as views for ``n``
        rows: reward (4 bytes a row) | done | truncated (1 each) side by side in one block, one copy."""
        if self._stage is None:
            rows = self.n_streams
            mk = lambda: (torch.zeros(6 * rows, dtype=torch.uint8, pin_memory=True),
                          torch.zeros(6 * rows, dtype=torch.uint8, device=self.device))
            self._stage = _Staging(lambda: dict(block=mk(), views={}))
        st = self._stage.acquire()
        v = st["views"].get(n)
        if v is None:
            cut = lambda t: dict(reward=t[0:4 * n].view(torch.float32), done=t[4 * n:5 * n], trunc=t[5 * n:6 * n])
            h, d = cut(st["block"][0]), cut(st["block"][1])
            v = {k: (h[k].numpy(), d[k]) for k in h}
            v["copy"] = (st["block"][1][:6 * n], st["block"][0][:6 * n])
            st["views"][n] = v
        return v

    def track(self, reward, done, truncated):
        """One environment step: row i is stream i.  NumPy arrays / host tensors travel through the pinned rotation, device
        tensors are used in place and never read by the host; nothing synchronises.  Rewards of any float dtype are
        narrowed to float32, ``done`` / ``truncated`` may be bool or uint8."""
        if not torch.is_tensor(reward):
            reward = np.asarray(reward)
        n = int(reward.reshape(-1).shape[0])
        if not 1 <= n <= self.n_streams:
            raise ValueError(f"EvalTracker.track: n = {n} rows must be in [1, n_streams = {self.n_streams}]")
        if self._quota is not None and n != self.n_streams:
            raise ValueError(f"EvalTracker.track: the quota rule speaks about every stream: n = {n} rows must be "
                             f"n_streams = {self.n_streams}")
        rows = [("reward", reward, torch.float32), ("done", done, torch.uint8), ("trunc", truncated, torch.uint8)]
        staged = not all(_is_dev(r[1]) for r in rows)
        with self._on_device:
            v = self._staging(n) if staged else {}
            dev = {k: _device_array(x, n, dtype, v.get(k))[0] for k, x, dtype in rows}
            if staged:
                v["copy"][0].copy_(v["copy"][1], non_blocking=True)
            if self._quota is None:
                N.check(N.lib().prism_eval_track(self._desc_ref, n, N.ptr(dev["reward"]), N.ptr(dev["done"]),
                                                 N.ptr(dev["trunc"]), N.current_stream_handle()), "prism_eval_track")
            else:
                N.check(N.lib().prism_eval_track_quota(self._desc_ref, self._quota_ref, n, N.ptr(dev["reward"]),
                                                       N.ptr(dev["done"]), N.ptr(dev["trunc"]), N.current_stream_handle()),
                        "prism_eval_track_quota")
            if staged:
                self._stage.submit()

    def closed(self):
        """Whether the evaluation takes no further step: the reference's loop condition, as the device has it after every
        call made so far.  One event wait, then the two pinned words the last launch wrote (under the quota rule: the one
        word that holds its closing predicate)."""
        with self._on_device:
            ev = torch.cuda.Event()
            ev.record()
            ev.synchronize()
        if self._quota is not None:
            return self._host_closed[0].item() != 0
        episodes, rows = self._host_counts.tolist()
        return rows >= self.budget and episodes >= 1

    def result(self):
        """What the evaluation has collected (one small device-to-host copy).  ``std`` is the population value, as
        ``np.std``: from the logged returns when every episode was logged, else from the two sums.  ``returns``: the
        logged returns, in (step, stream) order."""
        cap = self.log_capacity
        w = self._words.cpu()
        stats, counts = w[:4].view(torch.float64).tolist(), w[4:8].tolist()
        n = int(counts[0])
        returns = w[8:8 + cap].view(torch.float64)[:min(n, cap)].tolist()
        res = summarize(stats, counts, returns)
        if self._quota is not None:
            res.update(calls=int(counts[3]), incomplete_streams=self.n_streams - int(w[-2]),
                       episodes_per_stream=self.episodes_per_stream)
        return res


def summarize(stats, counts, returns):
    """The ``result()`` dict from the four sums, the four counts and the logged returns (plain Python numbers)."""
    n = int(counts[0])
    if n == 0:
        return dict(episodes=0, mean=None, std=None, min=None, max=None, mean_length=None, timesteps=int(counts[2]),
                    returns=[])
    mean = stats[0] / n
    if len(returns) == n:
        std = float(np.std(np.asarray(returns, np.float64)))
    else:
        std = math.sqrt(max(stats[1] / n - mean * mean, 0.0))
    return dict(episodes=n, mean=mean, std=std, min=stats[2], max=stats[3], mean_length=counts[1] / n,
                timesteps=int(counts[2]), returns=[float(r) for r in returns])


def check_evaluable(agent):
    """Refuse, before anything runs, an agent whose evaluation could not be kept apart from its training streams."""
    from prism_amd.agents.action_selectors import EGreedyActionSelector
    if getattr(agent, "tau_rng", "philox") == "torch":
        raise ValueError('evaluation needs tau_rng = "philox": with tau_rng = "torch" the quantile draws come from torch\'s '
                         "generator and cannot be set aside for an evaluation")
    if isinstance(agent.eval_action_selector, EGreedyActionSelector):
        raise ValueError("evaluation refuses an EGreedyActionSelector as eval_action_selector: every call would advance "
                         "its anneal")


class VectorEvaluator:
    """``SyncAgentEvaluator`` over N lock-stepped environments.  One evaluation: ``envs.reset()``, ``agent.eval()``, then
    per step one ``agent.forward``, one ``envs.step``, one ``tracker.track`` and ``envs.observe()``, and ``agent.train()``
    at the end, whatever happens.  A step contributes N timesteps; the episodes are listed in (step, stream) order and the
    ones still open at the end are dropped, as the reference drops its one.  The host counts the timesteps itself and asks
    the device (``EvalTracker.closed``) only once they have reached the horizon, then after every further step.

    ``episodes_per_env`` = E >= 1: the quota rule instead (``prism_eval_track_quota``), the one to use at any N > 1: every
    environment contributes exactly its first E finished episodes, and the evaluation closes when every one has, or after
    ``max_steps_per_env`` steps (None: E x the environments' ``episode_timestep_limit`` where they have a positive one,
    else ``evaluation_timestep_horizon``, per stream).  The host then asks the device every ``EVAL_QUOTA_POLL_STEPS``
    steps; the steps issued behind the closing call are taken by nobody, and the acting draws they consumed count into
    ``eval_draws``.  A cap that closes the evaluation with streams short of the quota warns, and ``last`` says how many
    (``incomplete_streams``).  0 (the default): the budget rule, the reference's."""

    def __init__(self, agent, envs, timesteps_between_evaluations, evaluation_timestep_horizon, log_capacity=4096,
                 episodes_per_env=0, max_steps_per_env=None):
        check_evaluable(agent)
        self.agent, self.envs = agent, envs
        self.episodes_per_env = int(episodes_per_env or 0)
        if self.episodes_per_env < 0:
            raise ValueError("VectorEvaluator: episodes_per_env must be >= 0")
        if max_steps_per_env is None and self.episodes_per_env:
            limit = int(getattr(envs, "episode_timestep_limit", 0) or 0)
            max_steps_per_env = self.episodes_per_env * limit if limit > 0 else int(evaluation_timestep_horizon)
        self.max_steps_per_env = int(max_steps_per_env) if self.episodes_per_env else 0
        if self.episodes_per_env and self.max_steps_per_env < 1:
            raise ValueError("VectorEvaluator: max_steps_per_env must be >= 1 under the quota rule")
        self.timesteps_between_evaluations = timesteps_between_evaluations
        self.evaluation_timestep_horizon = int(evaluation_timestep_horizon)
        self.log_capacity = int(log_capacity)
        self.timesteps_since_last_eval = np.inf
        self.eval_draws = 0          # acting draws of all evaluations so far: the next one starts at EVAL_DRAW_BASE + this
        self.evaluations = 0
        self.last = None
        self.tracker = None

    def maybe_evaluate_agent(self, ts_this_iter, cumulative_timesteps):
        self.timesteps_since_last_eval += ts_this_iter
        if self.timesteps_since_last_eval >= self.timesteps_between_evaluations:
            self.timesteps_since_last_eval = 0
            return self.evaluate_agent()
        return None

    def _tracker(self, n):
        t = self.tracker
        if t is None or t.n_streams != n or t.budget != self.evaluation_timestep_horizon:
            if self.episodes_per_env:
                t = EvalTracker(n, self.evaluation_timestep_horizon, self.log_capacity, self.agent.device,
                                episodes_per_stream=self.episodes_per_env, max_calls=self.max_steps_per_env)
            else:
                t = EvalTracker(n, self.evaluation_timestep_horizon, self.log_capacity, self.agent.device)
            self.tracker = t
        return t

    def evaluate_agent(self, verbose=False):
        """The returns of the episodes that ended, in (step, stream) order (the first ``log_capacity`` of them; ``self.last``
        has the statistics over all)."""
        agent, envs = self.agent, self.envs
        check_evaluable(agent)
        obs = envs.reset()
        n = int(obs.shape[0])
        tracker = self._tracker(n)
        tracker.reset()
        horizon, quota = self.evaluation_timestep_horizon, self.episodes_per_env
        stream = None
        agent.eval()
        try:
            with agent.acting_stream(EVAL_DRAW_BASE + self.eval_draws) as stream:
                steps = 0
                while True:
                    action = agent.forward(obs)
                    _, reward, done, truncated = envs.step(action)
                    tracker.track(reward, done, truncated)
                    obs = envs.observe()
                    steps += 1
                    if quota:
                        if steps % EVAL_QUOTA_POLL_STEPS == 0 and tracker.closed():
                            break
                    elif steps * n >= horizon and tracker.closed():
                        break
        finally:
            agent.train()
            if stream is not None:
                self.eval_draws = stream.count - EVAL_DRAW_BASE
        self.last = tracker.result()
        self.evaluations += 1
        if quota and self.last["incomplete_streams"] > 0:
            warnings.warn(f"prism_amd: the evaluation closed at its cap of {self.max_steps_per_env} steps per environment "
                          f"with {self.last['incomplete_streams']} of {n} environments short of their "
                          f"{quota} episodes; its mean leaves their missing episodes out")
        if verbose:
            for i, r in enumerate(self.last["returns"]):
                print(i + 1, r)
        return list(self.last["returns"])

    def state_dict(self):
        """Plain data for an exact-resume snapshot."""
        since = self.timesteps_since_last_eval
        st = dict(timesteps_since_last_eval="inf" if since == np.inf else (float(since) if since != int(since) else int(since)),
                  eval_draws=int(self.eval_draws), evaluations=int(self.evaluations), last=self.last)
        if self.episodes_per_env:          # (the keys exist only under the quota rule)
            st.update(episodes_per_env=self.episodes_per_env, max_steps_per_env=self.max_steps_per_env)
        return st

    def _compat_record(self):
        """What a snapshot must agree on with the evaluator it is restored into: the stopping rule."""
        return dict(episodes_per_env=self.episodes_per_env, max_steps_per_env=self.max_steps_per_env)

    def load_state_dict(self, state):
        from prism_amd.util import snapshot
        snapshot.check_compat(dict(episodes_per_env=state.get("episodes_per_env", 0),
                                   max_steps_per_env=state.get("max_steps_per_env", 0)), self._compat_record(),
                              "VectorEvaluator.load_state_dict")
        since = state["timesteps_since_last_eval"]
        self.timesteps_since_last_eval = np.inf if since == "inf" else since
        self.eval_draws, self.evaluations, self.last = int(state["eval_draws"]), int(state["evaluations"]), state["last"]

    def close(self):
        close = getattr(self.envs, "close", None)
        if close is not None:
            close()


def _checkpoint_timesteps(path):
    return int(path.rsplit("_", 1)[-1])


def complete_checkpoints(checkpoint_dir):
    """The directories ``agent_checkpoint_<timesteps>`` under ``checkpoint_dir`` that hold ``agent/model.pt``,
    ``optimizer.pt`` and ``state.pkl`` (a checkpoint still being written does not), the highest timestep count first."""
    found = []
    for name in os.listdir(checkpoint_dir):
        if not name.startswith("agent_checkpoint_") or not name.rsplit("_", 1)[-1].isdigit():
            continue
        path = os.path.join(checkpoint_dir, name)
        if all(os.path.exists(os.path.join(path, "agent", f)) for f in ("model.pt", "optimizer.pt", "state.pkl")):
            found.append(path)
    return sorted(found, key=_checkpoint_timesteps, reverse=True)


class CheckpointEvaluator:
    """``CheckpointAgentEvaluator``: evaluate every complete ``agent_checkpoint_<timesteps>`` directory under
    ``checkpoint_dir``, the highest timestep count first.  ``logger`` (optional) takes what the reference sends to wandb."""

    def __init__(self, config, checkpoint_dir, envs, logger=None, episodes_per_env=0, max_steps_per_env=None):
        from prism_amd.factory import agent_factory
        self.checkpoint_dir = checkpoint_dir
        self.unprocessed_checkpoints = []
        self.processed_checkpoints = []
        self.logger = logger
        self.agent = agent_factory.build_agent(config, tuple(int(s) for s in envs.obs_shape), int(envs.n_actions))
        self.evaluator = VectorEvaluator(self.agent, envs, 0, config.evaluation_timestep_horizon,
                                         episodes_per_env=episodes_per_env, max_steps_per_env=max_steps_per_env)

    def run_evals(self, break_after_all_checkpoints=True):
        import time
        while True:
            self.scan_checkpoints()
            if len(self.unprocessed_checkpoints) == 0:
                if break_after_all_checkpoints:
                    break
                time.sleep(1)
                continue
            checkpoint = self.unprocessed_checkpoints.pop(0)
            self.agent.load(checkpoint)
            print("Evaluating checkpoint", checkpoint)
            self.evaluator.evaluate_agent(verbose=False)
            last = self.evaluator.last
            if self.logger is not None:
                cumulative_timesteps = int(checkpoint[checkpoint.rfind("_") + 1:])
                self.logger.log_data(last["mean"], "Report/Rewards", "Eval Reward")
                if last.get("incomplete_streams"):
                    self.logger.log_data(last["incomplete_streams"], "Report/Rewards", "Eval Incomplete Streams")
                self.logger.log_data(cumulative_timesteps, "Report/Metrics", "Cumulative Timesteps")
            print("EVALUATION OF CHECKPOINT {} COMPLETE.\n"
                  "MEAN REWARD: {}\n"
                  "STD REWARD: {}\n".format(checkpoint, last["mean"], last["std"]))
            self.processed_checkpoints.append(checkpoint)

    def scan_checkpoints(self):
        new = [p for p in complete_checkpoints(self.checkpoint_dir)
               if p not in self.processed_checkpoints and p not in self.unprocessed_checkpoints]
        for path in new:
            print("Adding new checkpoint", path)
        if new:
            self.unprocessed_checkpoints.extend(new)
            self.unprocessed_checkpoints.sort(key=_checkpoint_timesteps, reverse=True)

    def close(self):
        self.evaluator.close()
