"""Host restatement, in plain numpy fp32, of the two ensemble-only selector kernels (prism_amd/csrc/act_ensemble.hip:
``prism_min_regret_select``, ``prism_simple_ids_select``; the arithmetic is stated in include/prism_hip.h).  Sums run
sequentially, in head order and in action order, every operation rounds to fp32 on its own (the library is built without
floating-point contraction).  tests/test_selectors_host.py holds it to the reference's recorded outputs; the GPU tests
use it where the fixture has no value of its own (the centred means of SimpleIDS)."""
import numpy as np

F = np.float32


def unsquish(name, y):
    """common.h ``unsquish_value`` on an fp32 array."""
    y = np.asarray(y, dtype=F)
    if name in (None, "none"):
        return y
    if name == "symlog":
        return (np.sign(y) * (np.exp(np.abs(y)) - F(1))).astype(F)
    if name == "obs_look_further":
        root = np.sqrt(F(1) + F(4 * 0.01) * (np.abs(y) + F(1) + F(0.01)))
        q = (root - F(1)) / F(2 * 0.01)
        return (np.sign(y) * (q * q - F(1))).astype(F)
    raise ValueError(name)


def ensemble_mean(q):
    """``q [n, A, heads]`` (unsquished): the mean over the heads, summed in head order."""
    s = np.zeros(q.shape[:2], dtype=F)
    for h in range(q.shape[2]):
        s = s + q[:, :, h]
    return s / F(q.shape[2])


def min_regret(q, lmbda, unsquish_name="none"):
    """``q [n, A, heads]`` fp32 -> dict(action [n], scores, mean, spread [n, A])."""
    q = unsquish(unsquish_name, q)
    heads = q.shape[2]
    assert heads >= 2
    mean = ensemble_mean(q)
    v = np.zeros_like(mean)
    for h in range(heads):
        d = q[:, :, h] - mean
        v = v + d * d
    spread = np.sqrt(v / F(heads - 1))
    sd = np.sqrt(spread)
    lm = F(lmbda)
    upper = (mean + lm * sd).max(axis=1, keepdims=True)
    regret = upper - (mean - lm * sd)
    scores = regret * regret
    assert scores.dtype == F
    return dict(action=scores.argmin(axis=1), scores=scores, mean=mean, spread=spread)


def simple_ids(q, beta, unsquish_name="none"):
    """``q [n, A, heads]`` fp32 -> dict(action [n], scores (the scaled values), mean, max_diff, q_values [n, A])."""
    q = unsquish(unsquish_name, q)
    mean = ensemble_mean(q)
    max_diff = q.max(axis=2) - q.min(axis=2)
    total = np.zeros(q.shape[0], dtype=F)
    for a in range(q.shape[1]):
        total = total + mean[:, a]
    q_values = mean - (total / F(q.shape[1]))[:, None]
    scores = F(1.0 - float(beta)) * max_diff + q_values * F(beta)
    assert scores.dtype == F
    return dict(action=scores.argmax(axis=1), scores=scores, mean=mean, max_diff=max_diff, q_values=q_values)
