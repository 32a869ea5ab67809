"""The byte observation ring's cases, shared by tests/test_obs_ring_host.py (shown on the CPU to reach what they are meant
for) and tests/test_gpu_obs_ring.py (the uint8 ring held to an fp32 twin bit for bit).  numpy only.

  * ``narrow`` -- the narrowing rule of ``prism_amd/csrc/common.h`` (obs_narrow) restated in NumPy;
  * ``Streams`` -- interleaved environment streams of byte-valued observations for ``extend_batch``, with seeded episode
    ends and truncations, and ``expected_ring``: the bytes the rows of a run leave in the ring's two arrays;
  * ``FUSED_CASES`` -- rings for the fused step (tests/replay_cases.py ``build_ring`` at capacity 64, the observations
    scaled to byte values beyond 1) and the successor class of a sampled slot as the front launch tells them apart."""
import collections
import functools

import numpy as np

from tests import helpers as H
from tests import replay_cases as R

# 25 words | 100 words | 250 of the front launch's 256 threads | not a multiple of four: the byte path of gather / insert / ingest
SHAPES = [(10, 10, 1), (10, 10, 4), (10, 10, 10), (6,)]
BYTE_VALUES = np.array([0, 0, 0, 0, 0, 1, 1, 1, 2, 37, 128, 254, 255], np.uint8)
# what a uint8 ring cannot hold: each alone in one row of the inexact-data tests
INEXACT = [0.5, -1.0, 256.0, float("nan"), -0.0]


def narrow(x):
    """obs_narrow over a float32 array: (byte stored, byte-exact?).  Byte-exact iff the bit pattern is that of float(b) for a
    b in 0..255; every other float is stored as 0."""
    f = np.ascontiguousarray(x, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        b = np.where((f >= 0) & (f <= 255), f, np.float32(0)).astype(np.uint8)
    exact = b.astype(np.float32).view(np.uint32) == f.view(np.uint32)
    return np.where(exact, b, np.uint8(0)).astype(np.uint8), exact


class Streams:
    """`n` environment streams stepped in lockstep: every ``step()`` is one ``extend_batch`` call's arguments (uint8
    observations).  A stream's next observation is the next row's observation while its episode goes on; about 9 % of the
    rows end an episode, 6 % are truncations."""

    def __init__(self, shape, n=8, seed=0):
        self.shape, self.n, self.rng = tuple(shape), n, np.random.default_rng(seed)
        self.cur = self._frames()

    def _frames(self):
        f = self.rng.choice(BYTE_VALUES, size=(self.n,) + self.shape)
        f.reshape(self.n, -1)[:, :3] = (0, 1, 255)                   # every row holds the three named values
        return f

    def step(self):
        n, rng = self.n, self.rng
        u = rng.random(n)
        done, trunc = u < 0.09, (u >= 0.09) & (u < 0.15)
        nxt = self._frames()
        out = dict(obs=self.cur, next_obs=nxt, action=rng.integers(0, 6, n).astype(np.int32),
                   reward=rng.standard_normal(n).astype(np.float32), done=done, truncated=trunc)
        self.cur = np.where((done | trunc).reshape((n,) + (1,) * len(self.shape)), self._frames(), nxt)
        return out


def expected_ring(capacity, steps, obs=None, succ=None, cursor=0):
    """The ring's two byte arrays after the rows of `steps` (in order, from `cursor`): a row without successor (done and not
    truncated) stores a zero successor row."""
    O = int(np.prod(steps[0]["obs"].shape[1:]))
    obs = np.zeros((capacity, O), np.uint8) if obs is None else obs
    succ = np.zeros((capacity, O), np.uint8) if succ is None else succ
    for st in steps:
        for i in range(st["obs"].shape[0]):
            obs[cursor] = st["obs"][i].reshape(-1)
            has_next = st["truncated"][i] or not st["done"][i]
            succ[cursor] = st["next_obs"][i].reshape(-1) if has_next else 0
            cursor = (cursor + 1) % capacity
    return obs, succ, cursor


# ---------------------------------------------------------------------------------------------- the fused step
FusedCase = collections.namedtuple("FusedCase", "C B use_per full seed")
FUSED_CAPACITY, FUSED_ROWS, FUSED_ROWS_FULL, FUSED_STEPS, FUSED_N_STEP = 64, 40, 64 + 24, 10, 3
# The seeds are chosen (on the CPU, tests/test_obs_ring_host.py holds them to it) so that the sampled slots include every
# successor class.  partial = 40 rows of 64 (eager steps); full = a ring written over (steps 3 .. 10 run from the hipGraph).
_SEEDS = {"per_c1_b2": 6, "per_c1_b16": 0, "per_c4_b2": 2, "per_c4_b16": 1, "per_c10_b2": 5, "per_c10_b16": 0,
          "uniform_c4_b2": 1, "uniform_c4_b16": 0, "per_c4_b16_full": 0, "per_c10_b2_full": 6, "uniform_c1_b16_full": 0}
FUSED_CASES = {}
for _C in (1, 4, 10):
    for _B in (2, 16):
        FUSED_CASES[f"per_c{_C}_b{_B}"] = FusedCase(_C, _B, True, False, _SEEDS[f"per_c{_C}_b{_B}"])
FUSED_CASES["uniform_c4_b2"] = FusedCase(4, 2, False, False, _SEEDS["uniform_c4_b2"])
FUSED_CASES["uniform_c4_b16"] = FusedCase(4, 16, False, False, _SEEDS["uniform_c4_b16"])
FUSED_CASES["per_c4_b16_full"] = FusedCase(4, 16, True, True, _SEEDS["per_c4_b16_full"])
FUSED_CASES["per_c10_b2_full"] = FusedCase(10, 2, True, True, _SEEDS["per_c10_b2_full"])
FUSED_CASES["uniform_c1_b16_full"] = FusedCase(1, 16, False, True, _SEEDS["uniform_c1_b16_full"])


def replay_case(case):
    rows = FUSED_ROWS_FULL if case.full else FUSED_ROWS
    return R.Case(FUSED_CAPACITY, rows, 3, FUSED_N_STEP, 0.99, case.C, case.B, case.use_per, 900 + case.seed)


@functools.lru_cache(maxsize=None)
def fused_ring(case):
    """(oracle ring, leaves, obs bytes, successor bytes): the boolean planes of ``R.build_ring`` scaled, element by element,
    to byte values up to 255 (the same scale in both arrays, so a successor row still equals the linked row)."""
    orc, prio = R.build_ring(replay_case(case))
    scale = np.random.default_rng(case.seed).choice(np.array([1, 1, 1, 2, 7, 255], np.uint8), size=orc.obs.shape[1])
    to_bytes = lambda x: (x.astype(np.uint8) * scale[None, :]).astype(np.uint8)
    return orc, prio, to_bytes(orc.obs), to_bytes(orc.succ_obs)


PRED, NONE, ELSEWHERE = "walk ends at the predicted slot", "no successor stored", "successor elsewhere"


def successor_class(orc, slot):
    """The three cases of the front launch's successor row (step_kernels.h, s_rec_state2 = 1, 2, 0): the row it asked for
    ahead of the walk -- slot + (n_step - 1) * (first link's stride), or the slot itself when the walk cannot start -- is
    the one the walk ends at; the walk ends on a row without successor; anything else (a dependent load)."""
    path, _, _, _ = R.walk(orc, slot)
    last = path[-1]
    if not int(orc.flags[last]) & 4:
        return NONE
    fl, nx = int(orc.flags[slot]), int(orc.link[slot])
    go = (fl & 4) and not (fl & 2) and orc.n_step > 1 and nx >= 0
    pred = slot + (orc.n_step - 1) * (nx - slot) if go else slot
    return PRED if 0 <= pred < orc.capacity and last == pred else ELSEWHERE


def known_indices(case, seed):
    """The slots the fused steps of a case sample, as far as the CPU can know them: every step of uniform replay (the Philox
    draws alone), the FIRST step of prioritized replay (the leaves the ring is installed with; later steps depend on the TD
    errors the network writes back).  `seed`: the buffer's (config.seed)."""
    orc, prio, _, _ = fused_ring(case)
    size = orc.length
    if not case.use_per:
        return np.concatenate([H.philox_uniform_index(seed, k * case.B, case.B, size) for k in range(FUSED_STEPS)])
    smp = R.fresh_sampler(replay_case(case), prio)
    mass = H.philox_per_mass(seed, 0, case.B, smp.sum_tree.query(0, size))
    return smp.sample(size, mass)[0]
