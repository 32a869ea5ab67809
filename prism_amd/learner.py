"""``Learner`` — same ``configure`` / ``learn`` surface as ``/root/reference/prism/learner.py``,
plus ``step()``: ONE pass of the hot section ``learner.py:95-125`` (sample -> IS weights -> TD
update -> priority writeback -> target sync) with everything resident in HBM.

Quirks kept on purpose: beta is forced to 0.5 every step (learner.py:104-107); the target network
is synced on a *timestep* period (learner.py:122-124).
"""
import os
import time
import warnings

import numpy as np

from prism_amd.factory import algorithm_factory

_TIMER_KEYS = ("Component Update Time", "Iteration Time", "Agent Update Time", "Batch Sampling Time",
               "Timestep Collection Time")


class Learner:
    def __init__(self):
        self.agent = self.timestep_collector = self.experience_buffer = self.logger = self.checkpointer = None
        self.evaluator = None
        self.cumulative_timesteps = 0
        self.cumulative_model_updates = 0
        self.timesteps_since_report = 0
        self.timesteps_since_target_model_update = 0
        self.collected_steps_per_second_ema = None
        self.overall_steps_per_second_ema = None
        self.loggables = {}
        self.per_beta = None
        self.time_phases = True
        self.fused = True
        self.hip_graph = True
        self.captured_loop = False
        self.graph_while_filling = False
        self.captured_iterations = 0
        self._captured = None
        self._resumed = False

    def configure(self, config, collector=None, obs_shape=None, n_actions=None, process_group=None, eval_envs=None):
        """``eval_envs`` (the ``VectorCollector`` protocol, prism_amd/collectors.py): evaluate the agent on them every
        ``config.timesteps_between_evaluations`` timesteps for ``config.evaluation_timestep_horizon`` timesteps
        (``VectorEvaluator``, prism_amd/evals.py); None: no evaluator, nothing else changes."""
        (self.agent, self.timestep_collector, self.experience_buffer, self.logger,
         self.checkpointer) = algorithm_factory.build_algorithm(config, collector, obs_shape, n_actions,
                                                                process_group)
        self.timestep_limit = config.timestep_limit
        self.initial_random_timesteps = config.num_initial_random_timesteps
        self.timesteps_per_iteration = config.timesteps_per_iteration
        self.timesteps_per_report = config.timesteps_per_report
        self.target_network_update_period = config.target_update_period
        self.use_target_network = config.use_target_network
        self.use_per = config.use_per
        if self.use_per:
            from prism_amd.util import LinearAnneal
            self.per_beta = LinearAnneal(config.per_beta_start, config.per_beta_end,
                                         config.per_beta_anneal_timesteps)
        self.cumulative_timesteps = self.cumulative_model_updates = 0
        self.timesteps_since_report = self.timesteps_since_target_model_update = 0
        self.reset_loggables()
        self.device = config.device
        # MI355X-only knobs (not Config fields): fuse the step into four launches / replay it from a hipGraph
        self.fused = bool(getattr(config, "fused_step", True)) and \
            getattr(config, "per_mass_rng", "philox") == "philox" and getattr(config, "tau_rng", "philox") == "philox"
        self.hip_graph = bool(getattr(config, "hip_graph", True))
        # ... / run a whole iteration (k x (act, environment step, ingest) + the step) as ONE hipGraph replay once its
        # conditions hold (prism_amd/captured_loop.py; off by default, and the loop is the eager one wherever they do not)
        self.captured_loop = bool(getattr(config, "captured_loop", False))
        # ... / replay the step, and the captured iteration, while the ring is still filling as well (the front launch
        # then reads the ring's size from the device; off by default)
        self.graph_while_filling = bool(getattr(config, "graph_while_filling", False))
        self.captured_iterations = 0
        self._captured = None
        self._resumed = False
        self.checkpointer.attach(self, config)              # config.backup_checkpoints: the hourly exact-resume snapshot
        self.evaluator = None
        if eval_envs is not None:
            from prism_amd.evals import VectorEvaluator
            # MI355X-only knobs, plain attributes like captured_loop: evaluation_episodes_per_env = E >= 1 evaluates by
            # episode quota per environment (the rule for any N > 1; 0, the default, is the reference's budget rule) and
            # evaluation_max_steps_per_env caps it (None: E x the environments' episode_timestep_limit where positive, else
            # evaluation_timestep_horizon, per stream)
            self.evaluator = VectorEvaluator(self.agent, eval_envs, config.timesteps_between_evaluations,
                                             config.evaluation_timestep_horizon,
                                             episodes_per_env=int(getattr(config, "evaluation_episodes_per_env", 0) or 0),
                                             max_steps_per_env=getattr(config, "evaluation_max_steps_per_env", None))

    # ------------------------------------------------------------------ the hot path
    def step(self, timesteps_this_iteration=0, eager=False):
        """learner.py:95-125.  All work is enqueued on the current HIP stream; nothing here
        synchronises with the device."""
        buf, agent, tp = self.experience_buffer, self.agent, self.time_phases
        if self.fused and hasattr(agent, "step_fused") and hasattr(buf, "flush"):
            buf.flush()
            if self.use_per:
                buf.buffer._sampler._beta = 0.5
            td = agent.step_fused(buf, eager=eager, use_graph=self.hip_graph, fill_graph=self.graph_while_filling)
            self._after_fused_update(timesteps_this_iteration)
            return td
        t0 = time.perf_counter() if tp else 0.0
        if self.cumulative_model_updates == 1 and agent.get_static_batch() is not None:
            buf.set_static_batch(agent.get_static_batch())
        batch, info = buf.sample(return_info=True)
        t1 = time.perf_counter() if tp else 0.0
        if self.use_per:
            per_weights = info["_weight"]
            buf.buffer._sampler._beta = 0.5
        else:
            per_weights = 1
        new_per_weights = agent.update(batch, per_weights=per_weights)
        self.cumulative_model_updates += 1
        t2 = time.perf_counter() if tp else 0.0
        if self.use_per:
            buf.update_priority(info["index"], new_per_weights, take_abs=True)
        self.timesteps_since_target_model_update += timesteps_this_iteration
        if self.use_target_network and self.timesteps_since_target_model_update >= self.target_network_update_period:
            agent.sync_target_model()
            self.timesteps_since_target_model_update = 0
        if tp:
            t3 = time.perf_counter()
            self.loggables["Batch Sampling Time"].append(t1 - t0)
            self.loggables["Agent Update Time"].append(t2 - t1)
            self.loggables["Component Update Time"].append(t3 - t2)
        return new_per_weights

    def _after_fused_update(self, timesteps_this_iteration):
        """Behind every fused update, eager or inside a captured iteration: the counters and the target sync on its
        timestep period (learner.py:122-124) -- an eager launch between two replays."""
        self.cumulative_model_updates += 1
        self.timesteps_since_target_model_update += timesteps_this_iteration
        if self.use_target_network and self.timesteps_since_target_model_update >= self.target_network_update_period:
            self.agent.sync_target_model()
            self.timesteps_since_target_model_update = 0

    # ------------------------------------------------------------------ the captured iteration (config.captured_loop)
    def _captured_iteration(self):
        """One iteration as one graph replay: the rows it collected, or None when the knob is off or this iteration has to
        run eagerly (``captured_loop_refusal``)."""
        if not self.captured_loop:
            return None
        if self._captured is None:
            from prism_amd.captured_loop import CapturedLoop
            self._captured = CapturedLoop(self)
        n = self._captured.run()
        if n is not None:
            self.captured_iterations += 1
            self._after_fused_update(n)
        return n

    def captured_loop_refusal(self):
        """Why the loop is not running as captured iterations, in one line (the condition that failed at the last iteration,
        or fails now if none has run); None when it is captured."""
        if not self.captured_loop:
            return "config.captured_loop is off"
        if self._captured is None:
            from prism_amd.captured_loop import CapturedLoop
            self._captured = CapturedLoop(self)
        return self._captured.reason if self._captured.judged else self._captured.check()[0]

    # ------------------------------------------------------------------ the outer loop
    def _learn(self):
        col = self.timestep_collector
        if not self._resumed:          # (after load_state the prologue has happened: its results came with the snapshot)
            self.cumulative_timesteps = col.collect_timesteps(self.initial_random_timesteps, self.agent,
                                                              self.experience_buffer, random=True)
            self.timesteps_since_report = self.cumulative_timesteps
            self.logger.set_holdout_data(self.experience_buffer.sample(return_info=False).clone())
            self.checkpointer.checkpoint(self.cumulative_timesteps)
        self._resumed = False
        while self.cumulative_timesteps < self.timestep_limit:
            loop_start = time.perf_counter()
            n = self._captured_iteration()
            captured = n is not None
            if captured:                       # collection and update were one replay: one timer, read at the bottom
                self.cumulative_timesteps += n
                self.timesteps_since_report += n
            else:
                n = col.collect_timesteps(self.timesteps_per_iteration, self.agent, self.experience_buffer)
                dt = time.perf_counter() - loop_start
                self.loggables["Timestep Collection Time"].append(dt)
                if n > 0:
                    self.cumulative_timesteps += n
                    self.timesteps_since_report += n
                    sps = n / dt
                    self.collected_steps_per_second_ema = sps if self.collected_steps_per_second_ema is None else \
                        self.collected_steps_per_second_ema * 0.9 + 0.1 * sps
                self.step(n)
            self.checkpointer.checkpoint(self.cumulative_timesteps)
            if self.evaluator is not None and \
                    self.evaluator.maybe_evaluate_agent(n, self.cumulative_timesteps) is not None:
                last = self.evaluator.last
                self.logger.log_data(last["mean"], "Report/Rewards", "Eval Reward")
                self.logger.log_data(last["episodes"], "Report/Rewards", "Eval Episodes")
                if last.get("incomplete_streams"):          # (quota rule only: the cap closed it)
                    self.logger.log_data(last["incomplete_streams"], "Report/Rewards", "Eval Incomplete Streams")
            if self.timesteps_since_report >= self.timesteps_per_report:
                self.report()
            it = time.perf_counter() - loop_start
            self.loggables["Iteration Time"].append(it)
            if n > 0:
                sps = n / it
                self.overall_steps_per_second_ema = sps if self.overall_steps_per_second_ema is None else \
                    self.overall_steps_per_second_ema * 0.9 + 0.1 * sps
                if captured:
                    self.collected_steps_per_second_ema = sps if self.collected_steps_per_second_ema is None else \
                        self.collected_steps_per_second_ema * 0.9 + 0.1 * sps

    def report(self):
        self._log()
        self.logger.report()
        self.timesteps_since_report = 0
        self.reset_loggables()

    def reset_loggables(self):
        self.loggables = {k: [] for k in _TIMER_KEYS}

    def _log(self):
        self.agent.log(self.logger)
        if self.timestep_collector is not None:
            self.timestep_collector.log(self.logger)
        if not self.loggables["Iteration Time"]:
            return
        if self.use_per:
            self.logger.log_data(self.per_beta.get_value(), "Report/PER", "Beta")
        self.logger.log_data(self.cumulative_timesteps, "Report/Metrics", "Cumulative Timesteps")
        self.logger.log_data(self.cumulative_model_updates, "Report/Model", "Number of Updates")
        self.logger.log_data(self.collected_steps_per_second_ema, "Report/Metrics", "Collected Steps per Second")
        self.logger.log_data(self.overall_steps_per_second_ema, "Report/Metrics", "Overall Steps per Second")
        for key, value in self.loggables.items():
            if value:
                self.logger.log_data(float(np.mean(value)), "Report/Metrics", key)

    def learn(self):
        if self.agent is None:
            print("YOU MUST CONFIGURE THE LEARNER BEFORE CALLING LEARN!")
            return
        if self.timestep_collector is None:
            raise RuntimeError("learn() needs a collector; use step() when feeding the buffer directly")
        finished = False
        try:
            self._learn()
            finished = True
        finally:
            try:
                self.checkpointer.save_backup_checkpoint()
            except Exception as e:          # noqa: BLE001 -- a snapshot that fails must not mask what ended the loop
                if finished:
                    raise
                warnings.warn(f"prism_amd: the backup checkpoint on the way out failed ({e!r})")
            finally:
                self.experience_buffer.empty()
                self.timestep_collector.close()
                if self.evaluator is not None:
                    self.evaluator.close()
                self.logger.close()

    # ------------------------------------------------------------------ exact resume (prism_amd/util/snapshot.py)
    def _snapshot_dir(self, path):
        """Rank-local: with more than one rank every rank writes and reads ``path/rank<r>``; no collective call."""
        if getattr(self.agent, "world", 1) > 1:
            import torch.distributed as dist
            return os.path.join(str(path), f"rank{dist.get_rank(self.agent.pg)}")
        return str(path)

    def _state_part(self):
        from prism_amd.util import snapshot

        def plain(b):
            return None if b is None else {k: plain(v) if isinstance(v, dict) else v.detach().cpu() for k, v in b.items()}

        opt = lambda x: None if x is None else float(x)
        hold = getattr(self.logger, "holdout_data", None)
        col = self.timestep_collector
        ev = {} if self.evaluator is None else dict(evaluator=self.evaluator.state_dict())      # (the key exists only then)
        return dict(
            **ev, cumulative_timesteps=int(self.cumulative_timesteps), cumulative_model_updates=int(self.cumulative_model_updates),
            timesteps_since_report=int(self.timesteps_since_report),
            timesteps_since_target_model_update=int(self.timesteps_since_target_model_update),
            collected_steps_per_second_ema=opt(self.collected_steps_per_second_ema),
            overall_steps_per_second_ema=opt(self.overall_steps_per_second_ema),
            per_beta=None if self.per_beta is None else self.per_beta.get_state(),
            last_agent_checkpoint_timesteps=int(self.checkpointer.last_agent_checkpoint_timesteps),
            holdout=plain(hold), holdout_batch_size=None if hold is None else getattr(hold, "batch_size", None),
            numpy_rng=snapshot.numpy_rng_state(), python_rng=snapshot.python_rng_state(),
            torch_rng=snapshot.torch_rng_state(), device_rng=snapshot.device_rng_state(self.agent.device),
            collector=col.state_dict() if hasattr(col, "state_dict") else None)

    def save_state(self, path):
        """One exact-resume snapshot of the whole run: the replay ring (part ``replay``), the agent (``agent/`` in the
        reference's layout + part ``agent_resume``) and the loop (part ``learner``: counters, target-sync timer, PER anneal,
        holdout batch, checkpoint mark, the global NumPy / Python / torch generators, the collector's ``state_dict()`` where
        it has one, the evaluator's where there is an evaluator).  Wall-clock timers are not part of it."""
        from prism_amd.util import snapshot
        agent, buf = self.agent, self.experience_buffer
        parts = {"replay": buf._state_part(), "agent_resume": agent._state_part(), "learner": self._state_part()}
        manifest = {"compat": {"replay": buf._compat_record(), "agent": agent._compat_record()}}
        if self.evaluator is not None and self.evaluator.episodes_per_env:          # (the record exists only under the quota rule)
            manifest["compat"]["evaluator"] = self.evaluator._compat_record()
        return snapshot.write_snapshot(self._snapshot_dir(path), parts, manifest, extra=agent.save)

    def load_state(self, path):
        """After ``configure()`` on fresh objects of the same configuration: put buffer, agent and loop back where
        ``save_state`` found them.  A following ``learn()`` skips its prologue (random collection, holdout sample, first
        checkpoint) and goes on with the loop; what it computes is bit-identical to the uninterrupted run."""
        from prism_amd.experience.hip_replay import Batch
        from prism_amd.util import snapshot
        agent, buf = self.agent, self.experience_buffer
        d = self._snapshot_dir(path)
        d = snapshot.latest(d) or d
        manifest = snapshot.read_manifest(d)
        agent._check_snapshot(manifest)          # every refusal comes before anything is touched
        buf._check_snapshot(manifest)
        stored = (manifest.get("compat") or {}).get("evaluator")
        if self.evaluator is not None and stored is not None:
            snapshot.check_compat(stored, self.evaluator._compat_record(), "Learner.load_state (evaluator)")
        parts, _ = snapshot.read_snapshot(d, ["replay", "agent_resume", "learner"])
        st = parts["learner"]
        if self.evaluator is not None and stored is None and st.get("evaluator") is not None:
            # an evaluator's state written under the budget rule: refused by an evaluator under the quota rule
            snapshot.check_compat(dict(episodes_per_env=0, max_steps_per_env=0), self.evaluator._compat_record(),
                                  "Learner.load_state (evaluator)")
        buf._restore_part(parts["replay"])
        agent._restore_part(d, parts["agent_resume"])
        for name in ("cumulative_timesteps", "cumulative_model_updates", "timesteps_since_report",
                     "timesteps_since_target_model_update", "collected_steps_per_second_ema",
                     "overall_steps_per_second_ema"):
            setattr(self, name, st[name])
        if self.per_beta is not None and st["per_beta"] is not None:
            self.per_beta.set_state(st["per_beta"])
        self.checkpointer.last_agent_checkpoint_timesteps = st["last_agent_checkpoint_timesteps"]
        if st["holdout"] is not None:
            B, dev = st["holdout_batch_size"], agent.device

            def batch(b):
                return Batch({k: batch(v) if isinstance(v, dict) else v.to(dev) for k, v in b.items()}, B, dev)
            self.logger.set_holdout_data(batch(st["holdout"]))
        col = self.timestep_collector
        if st["collector"] is not None and hasattr(col, "load_state_dict"):
            col.load_state_dict(st["collector"])
        if self.evaluator is not None and st.get("evaluator") is not None:
            self.evaluator.load_state_dict(st["evaluator"])
        # last: nothing above may draw from them
        snapshot.set_numpy_rng_state(st["numpy_rng"])
        snapshot.set_python_rng_state(st["python_rng"])
        snapshot.set_torch_rng_state(st["torch_rng"])
        snapshot.set_device_rng_state(st["device_rng"], agent.device)
        self.reset_loggables()
        self._resumed = True
