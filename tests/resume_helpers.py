"""Shared by tests/test_gpu_resume.py and the child process it starts (``python -m tests.resume_helpers``): the smallest
learner set-ups that still exercise every part of an exact-resume snapshot, a seeded scripted vector collector with a
``state_dict``, one loop iteration (``Agent.forward`` -> ``extend_batch`` -> ``Learner.step``) and the full state of a run.

Shapes: ring capacity 96 (tree capacity 128; not a power of two, and no multiple of the 5 lockstep streams, so the wrap is
not stream-aligned), batch 16, T = T' = 8, C = 4, A = 6, n-step 3."""
import contextlib
import copy
import io
import os
import sys

import numpy as np
import torch

CAPACITY, N_ENV, BATCH, C, A = 96, 5, 16, 4, 6
TARGET_PERIOD = 35                     # timesteps: every 7 iterations, never on a cut used by the tests

_EGREEDY = dict(use_e_greedy=True, e_greedy_decay_timesteps=100, e_greedy_final_epsilon=0.3)      # both coin sides happen
CASES = {
    # (a) IQN + PER + epsilon-greedy + Adam, a target network synchronised inside the window
    "a_iqn_per_egreedy_adam": dict(base=2, over=dict(_EGREEDY, use_target_network=True)),
    # (b) IDS + IQN + LayerNorm + target network, the action a Philox draw (ids_use_random_samples)
    "b_ids_sampled_full": dict(base=3, over=dict(ids_use_random_samples=True)),
    # (c) one-layer DQN head, uniform replay, centered RMSprop
    "c_dqn1_uniform_rmsprop": dict(base=0, over=dict(_EGREEDY, use_adam=False, use_rmsprop=True)),
    # parity modes: host NumPy priority masses, torch.rand quantile samples, the unfused sample / update path
    "parity_numpy_torch": dict(base=2, over=dict(_EGREEDY, use_target_network=True, per_mass_rng="numpy", tau_rng="torch")),
}


class ScriptedVectorCollector:
    """N lockstep environments whose transitions follow a seeded script: ONE ``Agent.forward`` and ONE ``extend_batch`` per
    step.  Everything it will do next follows from ``state_dict()`` (plain data)."""

    def __init__(self, n_env=N_ENV, n_channels=C, n_actions=A, seed=0, p_done=0.08, p_trunc=0.04):
        self.n_env, self.C, self.A, self.p_done, self.p_trunc = n_env, n_channels, n_actions, p_done, p_trunc
        self.rng = np.random.RandomState(seed)
        self.obs = None
        self.closed = False
        self.n_forward = 0
        self.last_actions = None

    def _obs(self):
        return self.rng.random_sample((self.n_env, 10, 10, self.C)) < 0.15

    def get_env_info(self):
        return (10, 10, self.C), self.A, 1

    def signal_processes_start_collecting(self, agent):
        pass

    def collect_timesteps(self, n_timesteps, agent, exp_buffer, random=False):
        if self.obs is None:
            self.obs = self._obs()
        got = 0
        while got < n_timesteps:
            if random:
                acts = self.rng.randint(0, self.A, self.n_env)
            else:
                acts = agent.forward(self.obs.astype(np.float32))
                self.n_forward += 1
                self.last_actions = acts.cpu().clone()
            rng = self.rng
            nxt = self._obs()
            done = rng.random_sample(self.n_env) < self.p_done
            trunc = ~done & (rng.random_sample(self.n_env) < self.p_trunc)
            exp_buffer.extend_batch(self.obs, nxt, acts, rng.standard_normal(self.n_env).astype(np.float32), done, trunc)
            self.obs = np.where((done | trunc)[:, None, None, None], self._obs(), nxt)
            got += self.n_env
        return got

    def state_dict(self):
        from prism_amd.util import snapshot
        return {"rng": snapshot.numpy_rng_state(self.rng), "n_forward": self.n_forward,
                "obs": None if self.obs is None else torch.from_numpy(self.obs.copy())}

    def load_state_dict(self, st):
        from prism_amd.util import snapshot
        snapshot.set_numpy_rng_state(st["rng"], self.rng)
        self.n_forward = int(st["n_forward"])
        self.obs = None if st["obs"] is None else st["obs"].numpy().copy()

    def log(self, logger):
        logger.log_data(data=0.0, group_name="Report/Rewards", var_name="Training Reward")

    def close(self):
        self.closed = True


def make_config(case, ckpt_dir, dev="cuda:0", **over):
    from prism_amd.config import baseline_config
    spec = CASES[case]
    kw = dict(device=dev, batch_size=BATCH, experience_replay_capacity=CAPACITY, n_step_returns_length=3,
              num_initial_random_timesteps=40, timesteps_per_iteration=N_ENV, timestep_limit=10 ** 9, timesteps_per_report=100,
              timesteps_between_evaluations=70, target_update_period=TARGET_PERIOD, checkpoint_dir=str(ckpt_dir),
              log_to_wandb=False, seed=77)
    kw.update(spec["over"])
    kw.update(over)
    return baseline_config(spec["base"], **kw)


def make_learner(case, ckpt_dir, dev="cuda:0", collector_seed=3, n_actions=A, **over):
    """Fresh objects of a case: ``(learner, collector)``, configured, nothing run yet."""
    from prism_amd.learner import Learner
    cfg = make_config(case, ckpt_dir, dev, **over)
    col = ScriptedVectorCollector(n_actions=n_actions, seed=collector_seed)
    ln = Learner()
    with contextlib.redirect_stdout(io.StringIO()):
        ln.configure(cfg, collector=col)
    return ln, col


def iterate(ln, col):
    """One iteration; what it computed, on the host: (actions, TD errors, the step's scalars)."""
    col.collect_timesteps(N_ENV, ln.agent, ln.experience_buffer)
    ln.cumulative_timesteps += N_ENV
    td = ln.step(N_ENV)
    return col.last_actions, td.cpu().clone(), ln.agent.scalars.cpu().clone()


def full_state(ln, col=None):
    """Everything a run has become, as host data: parameters and optimizer, the whole ring and both trees, host mirrors,
    the three counter totals, selector and loop state."""
    agent, buf = ln.agent, ln.experience_buffer
    buf.flush()
    torch.cuda.synchronize()
    st = {"flat": agent.flat.cpu().clone(), "opt_step": int(agent.optimizer.step_t.item()), "n_updates": agent.n_updates}
    if agent.flat_target is not None:
        st["flat_target"] = agent.flat_target.cpu().clone()
    for i, b in enumerate(agent.optimizer.buffers()):
        st[f"opt_buf{i}"] = b.cpu().clone()
    for name in ("obs", "succ_obs", "reward", "action", "flags", "link", "back", "tree", "per_state", "status"):
        t = getattr(buf, name)
        if t is not None:
            st["ring_" + name] = t.cpu().clone()
    st["batch_shapes"] = [list(buf._obs.shape), list(buf._next_obs.shape), list(buf._index.shape)]
    st["stream_tab"] = None if buf._stream_tab is None else buf._stream_tab.cpu().clone()
    st["slot_id"] = torch.from_numpy(buf._slot_id.copy())
    st["pending"] = sorted([int(k), int(v[0]), int(v[1])] for k, v in buf._pending.items())
    st["cursor"], st["size"], st["serial"] = int(buf.buffer._writer._cursor), int(buf._size), int(buf._serial)
    st["per_draws"] = int(buf._draws + buf._fused_draws)
    st["tau_draws"] = int(agent._draw_offset + agent._fused_tau)
    st["act_draws"] = int(agent._act_draws)
    st["sampler"] = [buf.buffer._sampler._alpha, buf.buffer._sampler._beta, buf.buffer._sampler._eps]
    sel = agent.action_selector
    if hasattr(sel, "rng"):                      # epsilon-greedy: the anneal step and the host generator of coin and actions
        st["eps_step"] = int(sel.epsilon.get_state())
        st["selector_next_draw"] = float(copy.deepcopy(sel.rng).uniform(0, 1))
    for name in ("cumulative_timesteps", "cumulative_model_updates", "timesteps_since_report",
                 "timesteps_since_target_model_update"):
        st[name] = int(getattr(ln, name))
    st["last_agent_checkpoint_timesteps"] = int(ln.checkpointer.last_agent_checkpoint_timesteps)
    if col is not None:
        st["collector_next_draw"] = float(copy.deepcopy(col.rng).uniform(0, 1))
        st["collector_obs"] = None if col.obs is None else torch.from_numpy(col.obs.copy())
    return st


def assert_same(got, want, where=""):
    """Bit-for-bit equality of two nested records (tensors with torch.equal on their bits: NaN-safe, -0.0 is not 0.0)."""
    if torch.is_tensor(want):
        assert torch.is_tensor(got) and got.dtype == want.dtype and got.shape == want.shape, where
        if want.dtype.is_floating_point:
            got, want = got.contiguous().view(torch.int32), want.contiguous().view(torch.int32)
        assert torch.equal(got, want), f"{where}: {int((got != want).sum())} of {want.numel()} values differ"
    elif isinstance(want, dict):
        assert isinstance(got, dict) and got.keys() == want.keys(), where
        for k in want:
            assert_same(got[k], want[k], f"{where}.{k}" if where else str(k))
    elif isinstance(want, (list, tuple)):
        assert isinstance(got, (list, tuple)) and len(got) == len(want), where
        for i, (g, w) in enumerate(zip(got, want)):
            assert_same(g, w, f"{where}[{i}]")
    else:
        assert got == want, f"{where}: {got!r} != {want!r}"


def child_main(case, snapshot_dir, n_iter, out_file, ckpt_dir):
    """The fresh-process leg: build the case's objects, restore, run, leave the records and the final state in a file."""
    ln, col = make_learner(case, ckpt_dir)
    ln.load_state(snapshot_dir)
    records = [iterate(ln, col) for _ in range(int(n_iter))]
    torch.save({"records": [list(r) for r in records], "state": full_state(ln, col)}, out_file)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    child_main(*sys.argv[1:6])
