"""Risk-sensitive acting: ``config.iqn_risk_policy_id`` (Dabney et al. 2018, "Implicit Quantile Networks for Distributional
Reinforcement Learning", section "Risk-sensitive reinforcement learning").

The reference leaves the knob unimplemented: its parser (``model_factory.py:10-13``) returns ``None`` for every id, behind a
hook in ``IQNModel.forward`` (``iqn_model.py:73-78``).  Here an id is ``"neutral"`` / ``None`` or ``"<name>:<eta>"``::

    cvar:eta   beta(tau) = eta * tau                                              0 < eta <= 1
    wang:eta   beta(tau) = Phi(Phi^-1(tau) + eta)                                 eta finite; eta < 0 is risk-averse
    cpw:eta    beta(tau) = tau^eta / (tau^eta + (1 - tau)^eta)^(1 / eta)          0 < eta <= 1
    pow:eta    beta(tau) = tau^(1 / (1 + |eta|))              for eta >= 0,
                           1 - (1 - tau)^(1 / (1 + |eta|))    for eta < 0         eta finite

beta is evaluated in float64 from the float32 sample and narrowed once to float32; every policy maps 0 to 0 and [0, 1] into
[0, 1].  Acting only: the agent embeds beta(tau) in place of tau in every acting forward (``prism_act_tau_distort`` in
front of ``prism_act_forward``, include/prism_hip.h; ``distort`` below is the same map in torch for ``IQNHead.forward``),
the update stays neutral.  The decision must read the quantile means, so a model with Q heads refuses a non-neutral id."""
import math

import torch

from prism_amd import _native as N

POLICIES = {"cvar": N.RISK_CVAR, "wang": N.RISK_WANG, "cpw": N.RISK_CPW, "pow": N.RISK_POW}
_NAMES = {v: k for k, v in POLICIES.items()}
NEUTRAL = (N.RISK_NEUTRAL, 0.0)


def parse(policy_id):
    """``(PRISM_RISK_* id, eta)`` of ``config.iqn_risk_policy_id``; ``ValueError`` for an unknown name, a missing or
    non-numeric eta, or an eta outside the policy's range."""
    if policy_id is None or policy_id == "neutral":
        return NEUTRAL
    if not isinstance(policy_id, str):
        raise ValueError(f"iqn_risk_policy_id must be a string or None, got {policy_id!r}")
    name, sep, arg = policy_id.partition(":")
    if name not in POLICIES:
        raise ValueError(f"iqn_risk_policy_id {policy_id!r}: unknown risk policy {name!r} "
                         f"('neutral' or one of {sorted(POLICIES)} as '<name>:<eta>')")
    if not sep or not arg.strip():
        raise ValueError(f"iqn_risk_policy_id {policy_id!r}: {name} needs its eta ('{name}:<eta>')")
    try:
        eta = float(arg)
    except ValueError:
        raise ValueError(f"iqn_risk_policy_id {policy_id!r}: eta {arg!r} is not a number") from None
    if not math.isfinite(eta):
        raise ValueError(f"iqn_risk_policy_id {policy_id!r}: eta must be finite")
    if name in ("cvar", "cpw") and not 0.0 < eta <= 1.0:
        raise ValueError(f"iqn_risk_policy_id {policy_id!r}: {name} takes 0 < eta <= 1")
    return POLICIES[name], eta


def for_config(config):
    """``parse`` of the configuration's id, refused where the acting decision would not read the quantile means: with Q
    heads (``use_ids`` / ``use_dqn``) the selectors act on the ensemble and z only feeds the IDS variance term."""
    risk = parse(getattr(config, "iqn_risk_policy_id", None))
    if risk[0] != N.RISK_NEUTRAL and (config.use_ids or config.use_dqn or not config.use_iqn):
        raise ValueError(f"iqn_risk_policy_id = {config.iqn_risk_policy_id!r} needs an IQN-only model: with Q heads "
                         "(use_ids / use_dqn) the action selectors act on the ensemble, not on the quantile means")
    return risk


def canonical_id(risk):
    """The id ``parse`` maps back to ``risk`` (what a snapshot's compatibility record carries)."""
    return "neutral" if risk[0] == N.RISK_NEUTRAL else f"{_NAMES[risk[0]]}:{risk[1]!r}"


def distort(taus, risk):
    """beta(taus) for float32 samples of any shape: float64 inside, narrowed once -- ``prism_act_tau_distort``'s
    arithmetic in torch."""
    policy, eta = risk
    if policy == N.RISK_NEUTRAL:
        return taus
    u = taus.to(torch.float64)
    if policy == N.RISK_CVAR:
        out = eta * u
    elif policy == N.RISK_WANG:
        # (Phi through erfc: torch.special.ndtr adds 1 to erf and loses the lower tail, where eta < 0 takes small samples)
        out = 0.5 * torch.special.erfc(-(torch.special.ndtri(u) + eta) / math.sqrt(2.0))
    elif policy == N.RISK_CPW:
        a, b = u ** eta, (1.0 - u) ** eta
        out = a / (a + b) ** (1.0 / eta)
    else:
        e = 1.0 / (1.0 + abs(eta))
        out = u ** e if eta >= 0.0 else 1.0 - (1.0 - u) ** e
    return out.to(torch.float32)
