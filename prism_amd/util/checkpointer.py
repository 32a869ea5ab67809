"""Checkpointer with the reference's interface and on-disk layout
(``/root/reference/prism/util/checkpointer.py:8-51``): an agent checkpoint
``<save_dir>/agent_checkpoint_<timesteps>/agent/{model.pt,optimizer.pt,target_model.pt,state.pkl}`` every
``timesteps_per_agent_checkpoint`` timesteps; the hourly backup checkpoint is disabled in the reference by an early
``return`` (:23-24) and is a no-op here too by default; ``load_checkpoint`` restores agent and experience buffer.

With ``config.backup_checkpoints`` set (a knob of this build, not a Config field) the backup checkpoint is an exact-resume
snapshot of the whole run, ``Learner.save_state(<save_dir>/backup_checkpoint)``, on the same hourly clock and on the way out
of ``learn()``; ``latest_backup()`` names the newest complete one for ``Learner.load_state``."""
import os
import time


class Checkpointer:
    def __init__(self, save_dir, agent, experience_buffer, timesteps_per_agent_checkpoint, hours_per_backup):
        self.save_dir = save_dir
        self.agent = agent
        self.experience_buffer = experience_buffer
        self.timesteps_per_agent_checkpoint = timesteps_per_agent_checkpoint
        self.last_backup_checkpoint_time = time.time()
        self.last_agent_checkpoint_timesteps = 0
        self.seconds_per_backup = hours_per_backup * 60 * 60
        self.learner = None
        self.backup_checkpoints = False

    def attach(self, learner, config):
        """``Learner.configure`` hands over what the backup checkpoint snapshots and whether the configuration asks for it."""
        self.learner = learner
        self.backup_checkpoints = bool(getattr(config, "backup_checkpoints", False))

    def backup_dir(self):
        return os.path.join(self.save_dir, "backup_checkpoint")

    def load_checkpoint(self, checkpoint_dir):
        self.agent.load(checkpoint_dir)
        self.experience_buffer.load(checkpoint_dir)

    def save_backup_checkpoint(self):
        if not self.backup_checkpoints or self.learner is None:
            return
        self.learner.save_state(self.backup_dir())

    def latest_backup(self):
        """The newest complete backup snapshot (what ``Learner.load_state`` takes), or None.  A write that was cut short
        leaves the one before it, under ``backup_checkpoint.prev``."""
        from prism_amd.util import snapshot
        base = self.backup_dir()
        if self.learner is not None and self.learner._snapshot_dir(base) != base:          # rank-local: base/rank<r>
            return base if snapshot.latest(self.learner._snapshot_dir(base)) is not None else None
        return snapshot.latest(base)

    def save_agent_checkpoint(self):
        path = os.path.join(self.save_dir, f"agent_checkpoint_{self.last_agent_checkpoint_timesteps}")
        self.agent.save(path)

    def checkpoint(self, timesteps):
        now = time.time()
        if now - self.last_backup_checkpoint_time > self.seconds_per_backup:
            self.save_backup_checkpoint()
            self.last_backup_checkpoint_time = now
        if timesteps - self.last_agent_checkpoint_timesteps >= self.timesteps_per_agent_checkpoint:
            self.last_agent_checkpoint_timesteps = timesteps
            self.save_agent_checkpoint()
