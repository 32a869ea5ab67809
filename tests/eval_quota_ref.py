"""``EvalQuotaHost``: ``prism_eval_track_quota`` (include/prism_hip.h) restated in plain Python floats for N streams -- the
checker of the device under the quota rule.  The rule is the project's own, so no recording pins it: it is checked against
a per-stream walk and, at N = 1 with the quota set to the episodes a recorded run finished, against the reference's
fixture (tests/test_eval_quota_host.py).  No part of ``prism_amd/`` uses it."""
import math

import numpy as np


class EvalQuotaHost:
    def __init__(self, n_streams, quota, max_calls=2 ** 62, log_capacity=4096):
        self.n_streams, self.quota, self.max_calls = int(n_streams), int(quota), int(max_calls)
        self.log_capacity = int(log_capacity)
        assert self.n_streams >= 1 and self.quota >= 1 and self.max_calls >= 1
        self.ep_return = [0.0] * self.n_streams
        self.ep_length = [0] * self.n_streams
        self.ep_done = [0] * self.n_streams
        self.log_return = [0.0] * self.log_capacity
        self.log_length = [0] * self.log_capacity
        self.stats = [0.0, 0.0, 0.0, 0.0]          # sum | sum of squares | min | max of the finished returns
        self.counts = [0, 0, 0, 0]                 # episodes | sum of their lengths | live rows taken | calls taken
        self.qcounts = [0, 0]                      # streams that have met the quota | unused

    def closed(self):
        return self.qcounts[0] >= self.n_streams or self.counts[3] >= self.max_calls

    def track(self, reward, done, truncated):
        """One call of n_streams rows, row i = stream i; False when the evaluation was closed and nothing was taken.  The
        rows of streams that have met the quota are never looked at."""
        assert len(reward) == self.n_streams
        if self.closed():
            return False
        st, c = self.stats, self.counts
        live_rows = 0
        for i in range(self.n_streams):
            if self.ep_done[i] >= self.quota:
                continue
            live_rows += 1
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
                self.ep_done[i] += 1
                if self.ep_done[i] == self.quota:
                    self.qcounts[0] += 1
            else:
                self.ep_return[i], self.ep_length[i] = ret, length
        c[2] += live_rows
        c[3] += 1
        return True

    def arrays(self):
        """Every array of the two descriptors, in the device's dtypes."""
        return dict(ep_return=np.array(self.ep_return, np.float64), ep_length=np.array(self.ep_length, np.int32),
                    ep_done=np.array(self.ep_done, np.int32),
                    log_return=np.array(self.log_return, np.float64), log_length=np.array(self.log_length, np.int32),
                    stats=np.array(self.stats, np.float64), counts=np.array(self.counts, np.int64),
                    qcounts=np.array(self.qcounts, np.int64))

    def returns(self):
        return self.log_return[:min(self.counts[0], self.log_capacity)]

    def result(self):
        """What ``EvalTracker.result()`` reports under the quota rule, from this object's words."""
        n = self.counts[0]
        extra = dict(calls=self.counts[3], incomplete_streams=self.n_streams - self.qcounts[0],
                     episodes_per_stream=self.quota)
        if n == 0:
            return dict(episodes=0, mean=None, std=None, min=None, max=None, mean_length=None, timesteps=self.counts[2],
                        returns=[], **extra)
        mean = self.stats[0] / n
        rets = self.returns()
        std = float(np.std(np.array(rets, np.float64))) if len(rets) == n else \
            math.sqrt(max(self.stats[1] / n - mean * mean, 0.0))
        return dict(episodes=n, mean=mean, std=std, min=self.stats[2], max=self.stats[3], mean_length=self.counts[1] / n,
                    timesteps=self.counts[2], returns=list(rets), **extra)


def run_script(host, reward, kind):
    """Feed a script ([steps][n] rewards, kinds 0 goes on | 1 done | 2 truncated | 3 both) step by step until the
    evaluation is closed or the script is used up.  Returns the calls taken."""
    k = 0
    while k < len(reward) and not host.closed():
        host.track(reward[k], kind[k] & 1, kind[k] & 2)
        k += 1
    return k
