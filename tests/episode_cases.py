"""The checker of the episode bookkeeping ``extend_batch`` does on the device (``prism_replay_ingest_tracked``): a plain
Python loop over Python floats, i.e. float64 in the order the reference's collector computes -- held to the live reference
through ``tests/golden/collector_bookkeeping.npz`` (test_episode_host.py), and the device is held to it
(test_gpu_episodes.py).  No part of ``prism_amd/`` uses it."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "collector_bookkeeping.npz")


def clamp_f32(r):
    """PRISM_CLIP_CLAMP on float32 values: r < -1 ? -1 : (r > 1 ? 1 : r) -- NaN and -0.0 fail both compares and pass."""
    r = np.asarray(r, np.float32)
    return np.where(r < np.float32(-1), np.float32(-1), np.where(r > np.float32(1), np.float32(1), r)).astype(np.float32)


class EpisodeHost:
    """Per stream: the running return and length of the open episode; over all: the finished-episode words.  ``step()``
    takes the timesteps in the order they reach the buffer."""

    def __init__(self, ema=0.9, count_first_step=False, clip=None):
        self.ema, self.count_first_step, self.clip = float(ema), bool(count_first_step), clip
        self.ret, self.length = {}, {}                     # stream -> float / int (absent = 0)
        self.training_reward = None
        self.episodes = self.sum_length = self.rows = 0
        self.sum_return = self.last_return = 0.0

    def stored(self, reward):
        """The reward as the ring stores it (float32)."""
        r = np.float32(reward)
        if self.clip == "dopamine_clamp":
            r = np.float32(-1) if r < np.float32(-1) else (np.float32(1) if r > np.float32(1) else r)
        return r

    def step(self, stream, reward, done, truncated):
        """One timestep: (stored reward, its episodic return, the training reward after it)."""
        r = float(np.float32(reward))                      # the raw reward, widened exactly
        had = self.length.get(stream, 0)
        ret = 0.0 if had == 0 and not self.count_first_step else r + self.ret.get(stream, 0.0)
        n = had + 1
        self.rows += 1
        if done or truncated:
            if self.episodes == 0:
                self.training_reward = ret
            else:
                self.training_reward = self.ema * self.training_reward + (1 - self.ema) * ret
            self.episodes += 1
            self.sum_length += n
            self.sum_return += ret
            self.last_return = ret
            self.ret[stream], self.length[stream] = 0.0, 0
        else:
            self.ret[stream], self.length[stream] = ret, n
        return self.stored(reward), ret, self.training_reward

    def step_batch(self, ids, reward, done, truncated, untracked=()):
        """One extend_batch call, rows in order; the rows listed in ``untracked`` (stored unlinked) are skipped."""
        for i, e in enumerate(ids):
            if i not in untracked:
                self.step(int(e), reward[i], bool(done[i]), bool(truncated[i]))

    def close(self, stream=None):
        """A stream (or every stream) loses its open episode: empty(), a bulk load, a repeated id."""
        if stream is None:
            self.ret.clear()
            self.length.clear()
        else:
            self.ret[stream], self.length[stream] = 0.0, 0

    def stats(self):
        n = self.episodes
        return dict(episodes=n, training_reward=self.training_reward if n else None,
                    mean_return=self.sum_return / n if n else None, mean_length=self.sum_length / n if n else None,
                    last_return=self.last_return if n else None, rows=self.rows)

    def accumulators(self, size):
        """(ep_return float64 [size], ep_length int32 [size]) as the device holds them."""
        ret, length = np.zeros(size, np.float64), np.zeros(size, np.int32)
        for e, v in self.ret.items():
            if e < size:
                ret[e], length[e] = v, self.length[e]
        return ret, length


def bits64(x):
    return np.asarray(x, np.float64).view(np.int64)


def bits32(x):
    return np.asarray(x, np.float32).view(np.int32)
