"""``VectorCollector`` -- the collector ``Learner.learn()`` drives, over N environments stepped in lockstep: ONE
``Agent.forward`` and ONE ``extend_batch`` per environment step (the loop of INTEGRATION.md section 1).  It stands where the
reference has ``ExperienceCollector`` (``/root/reference/multiprocessing_experience_collection/experience_collector.py``):
same surface, no processes, no ``Timestep`` objects.  Reward clipping, the episodic returns and the training-reward EMA
the reference's collector computes on the host (``collector_process_interface.py:129-139``,
``experience_collector.py:113-118``) happen on the device inside ``extend_batch``'s launch
(``HipReplayBuffer.track_episodes``): arrays the environment hands over as device tensors are never read by the host.

``envs`` is any object with

    reset() -> obs [N, ...]                    start every environment
    step(actions) -> (next_obs, reward, done, truncated)
                                               next_obs[i]: what the step returned, BEFORE any auto-reset
    observe() -> obs [N, ...]                  the observations to act on next (a fresh one where an episode ended)
    n_actions, obs_shape                       attributes

Arrays are NumPy arrays or device tensors and are passed through untouched.
"""
import numpy as np


class VectorCollector:
    def __init__(self, envs, config, seed=None):
        self.envs = envs
        self.ema = float(getattr(config, "training_reward_ema", 0.9))
        self.seed = int(getattr(config, "seed", 0) if seed is None else seed)
        self.rng = np.random.default_rng(self.seed)          # the collector's own: random=True draws actions from it
        self.rows = 0
        self._obs = None
        self._started = False          # reset() has happened (or a restored run goes on: observe() instead)
        self._buffer = None

    def get_env_info(self):
        """(obs_shape, n_actions, n_agents), as ExperienceCollector.get_env_info."""
        return tuple(int(s) for s in self.envs.obs_shape), int(self.envs.n_actions), 1

    def signal_processes_start_collecting(self, agent):
        """There are no processes to signal; the environments are reset at the first collection."""

    def collect_timesteps(self, n_timesteps, agent, exp_buffer, random=False):
        """Whole environment steps until at least ``n_timesteps`` rows are stored; returns the rows stored.  ``random``:
        uniform actions from the collector's generator instead of ``agent.forward``."""
        envs = self.envs
        self._begin(exp_buffer)
        got = 0
        while got < n_timesteps:
            obs = self._obs
            n = int(obs.shape[0])
            action = self.rng.integers(0, int(envs.n_actions), n) if random else agent.forward(obs)
            next_obs, reward, done, truncated = envs.step(action)
            exp_buffer.extend_batch(obs, next_obs, action, reward, done, truncated)
            self._obs = envs.observe()
            got += n
        self.rows += got
        return got

    def _begin(self, exp_buffer):
        """What comes before the first environment step into ``exp_buffer``: episode tracking on, and the observations to act
        on -- a reset, or (a restored run goes on) what the environments show."""
        if self._buffer is not exp_buffer:
            exp_buffer.track_episodes(self.ema)
            self._buffer = exp_buffer
        if self._obs is None:
            self._obs = self.envs.observe() if self._started else self.envs.reset()
            self._started = True

    def log(self, logger):
        """The reference's "Training Reward" (None until the first episode has ended) and the episode count: one small
        device-to-host copy per report."""
        st = self._buffer.episode_stats() if self._buffer is not None else dict(training_reward=None, episodes=0)
        logger.log_data(data=st["training_reward"], group_name="Report/Rewards", var_name="Training Reward")
        logger.log_data(data=st["episodes"], group_name="Report/Rewards", var_name="Episodes")

    def state_dict(self):
        """Plain data for an exact-resume snapshot: the action generator and the row count, and under ``envs`` the
        environments' own ``state_dict()`` where they have one (prism_amd/envs.py).  The state of any other environments is
        their own business (as it is for the reference's environment processes): a caller that can restore it gets a
        bit-identical continuation, the collector goes on from ``envs.observe()``; one that cannot restores the ring with
        ``keep_streams=False``."""
        state = dict(rng=_plain(self.rng.bit_generator.state), rows=int(self.rows), started=bool(self._started))
        if hasattr(self.envs, "state_dict"):          # (the key exists only then: environments that restore themselves)
            state["envs"] = self.envs.state_dict()
        return state

    def load_state_dict(self, state):
        self.rng.bit_generator.state = state["rng"]
        self.rows, self._started = int(state["rows"]), bool(state["started"])
        self._obs = None
        if "envs" in state and hasattr(self.envs, "load_state_dict"):
            self.envs.load_state_dict(state["envs"])

    def close(self):
        close = getattr(self.envs, "close", None)
        if close is not None:
            close()


def _plain(x):
    """A bit generator's state as dicts / ints / strs only."""
    if isinstance(x, dict):
        return {k: _plain(v) for k, v in x.items()}
    if isinstance(x, (np.integer,)):
        return int(x)
    return x
