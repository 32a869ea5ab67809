"""Host restatement of epsilon-greedy action selection per observation (``prism_egreedy_select``, include/prism_hip.h):
plain numpy on top of ``tests/helpers.py::philox4x32`` and ``tests/select_ref.py::u64_to_unit_double``.

    s0      rows seen before the call (the selector's epsilon.current_step); the call has n_call rows
    eps     = anneal(start, stop, max_steps, s0 + n_call)            ONE value per call, float64
    r_b     = Philox4x32-10(seed, s0 + row, "EGRD"), row = row0 + b
    u_b     = u64_to_unit_double(r_b[0], r_b[1])
    action  = (r_b[2] * A) >> 32 if u_b < eps else the greedy action
"""
import numpy as np

from tests import helpers as H
from tests import select_ref as S

EGREEDY_KEY = 0x45475244          # "EGRD"


def anneal(start, stop, max_steps, step):
    """LinearAnneal.get_value() at ``current_step == step`` (prism/util/annealing_strategies.py:22-33), restated: the
    operations and their order are the class's, in float64."""
    if max_steps == 0 or step >= max_steps:
        return stop
    f = min(1, step / max_steps)
    return start * (1 - f) + stop * f


def draws(seed, s0, row0, n, n_actions):
    """Rows row0 .. row0 + n - 1 of the call that started at count ``s0``: (coins float64 [n], random actions int64 [n])."""
    ctr = np.uint64(s0) + np.uint64(row0) + np.arange(int(n), dtype=np.uint64)
    r = H.philox4x32(int(seed), ctr, EGREEDY_KEY)
    coins = S.u64_to_unit_double(r[:, 0], r[:, 1])
    random_actions = ((r[:, 2].astype(np.uint64) * np.uint64(n_actions)) >> np.uint64(32)).astype(np.int64)
    return coins, random_actions


def select(greedy, seed, s0, row0, n_call, n_actions, start, stop, max_steps, coins=None):
    """``(actions int64 [n], explored uint8 [n], eps)`` of rows row0 .. row0 + len(greedy) - 1 of a call of ``n_call`` rows;
    ``coins``: given uniforms of the WHOLE call (the kernel's u_in), indexed by row."""
    greedy = np.asarray(greedy, dtype=np.int64)
    n = greedy.shape[0]
    eps = anneal(start, stop, max_steps, int(s0) + int(n_call))
    u, rand = draws(seed, s0, row0, n, n_actions)
    if coins is not None:
        u = np.asarray(coins, dtype=np.float64)[row0:row0 + n]
    explored = u < eps
    return np.where(explored, rand, greedy).astype(np.int64), explored.astype(np.uint8), eps


def call_ranges(s0, calls):
    """Counter ranges ``[s, s + n)`` of a sequence of calls of n rows each from count ``s0``, and the count after them."""
    out = []
    for n in calls:
        out.append((s0, s0 + n))
        s0 += n
    return out, s0
