"""``EvalHost``: ``prism_eval_track`` (include/prism_hip.h) restated in plain Python floats for N streams -- the checker of
the device, itself checked against what the live reference's ``SyncAgentEvaluator`` recorded in
``tests/golden/evaluator_runs.npz`` (tests/test_eval_host.py).  No part of ``prism_amd/`` uses it."""
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "evaluator_runs.npz")


def bits64(x):
    return np.asarray(x, np.float64).view(np.uint64)


class EvalHost:
    def __init__(self, n_streams, budget, log_capacity=4096):
        self.n_streams, self.budget, self.log_capacity = int(n_streams), int(budget), int(log_capacity)
        self.ep_return = [0.0] * self.n_streams
        self.ep_length = [0] * self.n_streams
        self.log_return = [0.0] * self.log_capacity
        self.log_length = [0] * self.log_capacity
        self.stats = [0.0, 0.0, 0.0, 0.0]          # sum | sum of squares | min | max of the finished returns
        self.counts = [0, 0, 0, 0]                 # episodes | sum of their lengths | rows taken | calls taken

    def closed(self):
        """The reference's loop condition ``collected_ts < n_ts or len(ep_rews) == 0``, negated."""
        return self.counts[2] >= self.budget and self.counts[0] >= 1

    def track(self, reward, done, truncated):
        """One call of n rows, row i = stream i; False when the evaluation was closed and nothing was taken."""
        n = len(reward)
        assert 1 <= n <= self.n_streams
        if self.closed():
            return False
        st, c = self.stats, self.counts
        for i in range(n):
            length = self.ep_length[i] + 1
            ret = float(np.float32(reward[i])) + self.ep_return[i]
            if bool(done[i]) or bool(truncated[i]):
                self.ep_return[i], self.ep_length[i] = 0.0, 0
                if c[0] < self.log_capacity:
                    self.log_return[c[0]], self.log_length[c[0]] = ret, length
                sq = ret * ret
                st[0] += ret
                st[1] += sq
                if c[0] == 0:
                    st[2] = st[3] = ret
                else:
                    if ret < st[2]:
                        st[2] = ret
                    if ret > st[3]:
                        st[3] = ret
                c[0] += 1
                c[1] += length
            else:
                self.ep_return[i], self.ep_length[i] = ret, length
        c[2] += n
        c[3] += 1
        return True

    def arrays(self):
        """Every array of the descriptor, in the device's dtypes."""
        return dict(ep_return=np.array(self.ep_return, np.float64), ep_length=np.array(self.ep_length, np.int32),
                    log_return=np.array(self.log_return, np.float64), log_length=np.array(self.log_length, np.int32),
                    stats=np.array(self.stats, np.float64), counts=np.array(self.counts, np.int64))

    def returns(self):
        return self.log_return[:min(self.counts[0], self.log_capacity)]

    def result(self):
        """What ``EvalTracker.result()`` reports, from this object's words."""
        n = self.counts[0]
        if n == 0:
            return dict(episodes=0, mean=None, std=None, min=None, max=None, mean_length=None, timesteps=self.counts[2],
                        returns=[])
        mean = self.stats[0] / n
        rets = self.returns()
        std = float(np.std(np.array(rets, np.float64))) if len(rets) == n else \
            math.sqrt(max(self.stats[1] / n - mean * mean, 0.0))
        return dict(episodes=n, mean=mean, std=std, min=self.stats[2], max=self.stats[3], mean_length=self.counts[1] / n,
                    timesteps=self.counts[2], returns=list(rets))


def run_script(host, reward, kind, horizon_steps=None):
    """Feed a script ([steps][n] rewards, kinds 0 goes on | 1 done | 2 truncated | 3 both) the way ``VectorEvaluator``
    does: step by step until the evaluation is closed.  Returns the steps taken."""
    k = 0
    while not host.closed():
        host.track(reward[k], kind[k] & 1, kind[k] & 2)
        k += 1
    return k


def fixture_runs():
    g = np.load(GOLDEN)
    return {str(n): dict(reward=g[f"{n}_reward"], kind=g[f"{n}_kind"], horizon=int(g[f"{n}_horizon"]),
                         ep_rews_bits=g[f"{n}_ep_rews_bits"], timesteps=int(g[f"{n}_timesteps"])) for n in g["names"]}


class ScriptedEnvs:
    """N lock-stepped environments whose rewards and ends follow a script and do not depend on the action; records the
    actions it receives.  ``device``: hand reward / done / truncated over as device tensors."""

    def __init__(self, reward, kind, obs_shape=(10, 10, 4), n_actions=6, device=None, fail_at=None, seed=3):
        self.reward, self.kind = np.asarray(reward), np.asarray(kind)
        self.n = self.reward.shape[1]
        self.obs_shape, self.n_actions, self.device, self.fail_at = tuple(obs_shape), n_actions, device, fail_at
        rng = np.random.default_rng(seed)
        self._frames = rng.random((16, self.n) + self.obs_shape).astype(np.float32)
        self.k, self.resets, self.actions, self.closed = 0, 0, [], False

    def _obs(self):
        return self._frames[self.k % 16]

    def reset(self):
        self.k, self.resets = 0, self.resets + 1
        self.actions = []
        return self._obs()

    def observe(self):
        return self._obs()

    def step(self, action):
        if self.fail_at is not None and self.k == self.fail_at:
            raise RuntimeError("scripted failure")
        self.actions.append(np.asarray(action.cpu() if hasattr(action, "cpu") else action).copy())
        k = self.k
        self.k += 1
        r, d, t = self.reward[k], (self.kind[k] & 1).astype(bool), (self.kind[k] & 2).astype(bool)
        if self.device is not None:
            import torch
            r, d, t = (torch.as_tensor(x).to(self.device) for x in (r, d, t))
        return self._obs(), r, d, t

    def close(self):
        self.closed = True
