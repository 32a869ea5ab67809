"""Host restatement of sampled information-directed action selection (``prism_ids_sample_select``, include/prism_hip.h):
plain numpy on top of ``tests/helpers.py::philox4x32``; the clamped softmax alone is evaluated by torch on the CPU in fp32,
as the reference's selector evaluates it (action_selectors.py:150-152).

    p_a    = clamp(softmax(-scores)_a, eps, 1)                      fp32, not renormalised
    u_b    = u64_to_unit_double(Philox4x32-10(seed, c0 + b, "IDSA")[0:2])
    action = first a with u * S < p_0 + ... + p_a   (float64, index order; S = p_0 + ... + p_(A-1); A - 1 if none)
"""
import numpy as np
import torch

from tests import helpers as H

IDS_KEY = 0x49445341          # "IDSA"


def u64_to_unit_double(hi, lo):
    """common.h::u64_to_unit_double: 27 + 26 bits of two words as a float64 in [0, 1) (every step exact)."""
    a = (np.asarray(hi, dtype=np.uint32) >> np.uint32(5)).astype(np.float64)
    b = (np.asarray(lo, dtype=np.uint32) >> np.uint32(6)).astype(np.float64)
    return (a * 67108864.0 + b) / 9007199254740992.0


def ids_uniforms(seed, c0, n):
    """The uniforms of observations 0 .. n - 1 of the call whose forward started at acting count ``c0``."""
    r = H.philox4x32(int(seed), np.uint64(c0) + np.arange(int(n), dtype=np.uint64), IDS_KEY)
    return u64_to_unit_double(r[:, 0], r[:, 1])


def clamped_probs(scores, eps):
    """softmax(-scores).clamp(min=eps, max=1) in torch-CPU fp32: float32 array [n, A]."""
    s = torch.as_tensor(np.asarray(scores, dtype=np.float32))
    return torch.softmax(-s, dim=-1).clamp(min=eps, max=1).numpy()


def inverse_cdf(probs, u):
    """probs float32 [n, A] (or [A], shared by all draws), u float64 [n]: int64 [n]."""
    u = np.asarray(u, dtype=np.float64)
    p = np.asarray(probs, dtype=np.float32).astype(np.float64)
    if p.ndim == 1:
        p = np.broadcast_to(p, (u.shape[0], p.shape[0]))
    cum = np.zeros_like(p)
    acc = np.zeros(p.shape[0], dtype=np.float64)
    for a in range(p.shape[1]):          # (index order, one addition per action: the kernel's own chain)
        acc = acc + p[:, a]
        cum[:, a] = acc
    t = u * cum[:, -1]
    hit = t[:, None] < cum
    return np.where(hit.any(axis=1), hit.argmax(axis=1), p.shape[1] - 1).astype(np.int64)


def sample_actions(probs, seed, c0):
    probs = np.asarray(probs, dtype=np.float32)
    return inverse_cdf(probs, ids_uniforms(seed, c0, probs.shape[0]))


def call_ranges(c0, calls):
    """Counter ranges of a sequence of acting calls ``(n, T)`` from acting count ``c0``: per call the sampled selector's
    ``[c, c + n)`` -- c the count at the start of the call's forward -- and the count after it (``c + n * T``)."""
    out = []
    for n, T in calls:
        out.append((c0, c0 + n))
        c0 += n * T
    return out, c0
