"""Host restatement of the risk policies of ``config.iqn_risk_policy_id`` (prism_amd/agents/risk_policies.py,
``prism_act_tau_distort`` in include/prism_hip.h): the four distortions beta in NumPy float64, from float32 samples, narrowed
once to float32.  Phi^-1 is ``torch.special.ndtri`` in float64, Phi is stated through ``erfc`` (``_ndtr`` says why).  The
raw samples of an acting pass are ``tests/helpers.py philox_taus(seed, offset, T, n, TAU_ACT)``."""
import math

import numpy as np
import torch

from tests import helpers as H

NEUTRAL, CVAR, WANG, CPW, POW = 0, 1, 2, 3, 4
NAMES = {"cvar": CVAR, "wang": WANG, "cpw": CPW, "pow": POW}


def _ndtr(x):
    """Phi(x) = erfc(-x / sqrt(2)) / 2 in float64.  Not ``torch.special.ndtr``: that adds 1 to erf and loses the lower tail
    to cancellation (2.4e-7 relative at x = -7.3, where Wang with eta = -2 takes the sample 2^-24); through erfc the value
    is within 2e-14 relative of the exact one over the float32 samples (checked against 40-digit arithmetic)."""
    x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))
    return (0.5 * torch.special.erfc(-x / math.sqrt(2.0))).numpy()


def _ndtri(x):
    return torch.special.ndtri(torch.from_numpy(np.ascontiguousarray(x, dtype=np.float64))).numpy()


def beta64(policy, eta, tau):
    """beta(tau) in float64, before the narrowing."""
    u = np.asarray(tau, dtype=np.float32).astype(np.float64)
    eta = float(eta)
    if policy == NEUTRAL:
        return u
    if policy == CVAR:
        return eta * u
    if policy == WANG:
        with np.errstate(divide="ignore"):
            return _ndtr(_ndtri(u) + eta)
    if policy == CPW:
        a, b = np.power(u, eta), np.power(1.0 - u, eta)
        return a / np.power(a + b, 1.0 / eta)
    if policy == POW:
        e = 1.0 / (1.0 + abs(eta))
        return np.power(u, e) if eta >= 0.0 else 1.0 - np.power(1.0 - u, e)
    raise ValueError(policy)


def beta(policy, eta, tau):
    """beta(tau) as the kernel leaves it: float32."""
    return beta64(policy, eta, tau).astype(np.float32)


def raw_taus(seed, offset, T, n):
    """The raw samples of one acting pass of n observations at draw count ``offset``: float32[T * n], tau-major."""
    return H.philox_taus(seed, offset, T, n, H.TAU_ACT)


def ulp_distance(a, b):
    """Distance in float32 units in the last place between two arrays of non-negative floats (their bit patterns are
    ordered like the values)."""
    a = np.asarray(a, dtype=np.float32).view(np.int32).astype(np.int64)
    b = np.asarray(b, dtype=np.float32).view(np.int32).astype(np.int64)
    return np.abs(a - b)
