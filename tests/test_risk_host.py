"""CPU: ``config.iqn_risk_policy_id`` -- the parser and its refusals (prism_amd/agents/risk_policies.py, agent_factory), the
properties of the host restatement of the four distortions (tests/risk_ref.py), the torch form ``IQNHead.forward`` applies,
and ``prism_act_tau_distort``: declared, exported, bound, its argument checks and its kernel's private segment.
tests/test_gpu_risk.py holds the kernel and the agent to the restatement."""
import math
import os
import re

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import risk_ref as R

ETAS = {R.CVAR: (0.1, 0.25, 1.0), R.WANG: (-2.0, -0.75, 0.0, 0.75), R.CPW: (0.1, 0.25, 0.5, 0.71, 1.0),
        R.POW: (-2.0, -0.75, 0.0, 0.75)}
# Tversky and Kahneman's weighting function is increasing only for eta above 0.279 (Rieger and Wang 2006; Ingersoll 2008):
# below it the function dips just above 0.  Monotonicity is held where the function has it.
CPW_MONOTONE_FROM = 0.279


def _grid():
    """float32 samples in [0, 1): the ends 0, 2^-24 and 1 - 2^-24, every multiple of 2^-10, 4096 24-bit draws."""
    rng = np.random.default_rng(11)
    draws = (rng.integers(0, 2 ** 24, 4096).astype(np.float32) * np.float32(2.0 ** -24))
    g = np.concatenate([np.float32([0.0, 2.0 ** -24, 2.0 ** -23, 1.0 - 2.0 ** -24, 1.0 - 2.0 ** -23, 0.5]),
                        np.arange(1024, dtype=np.float32) / np.float32(1024), draws])
    return np.unique(g)          # (sorted)


def test_parser_accepts():
    from prism_amd import _native as N
    from prism_amd.agents import risk_policies as P
    assert P.parse(None) == P.parse("neutral") == P.NEUTRAL == (N.RISK_NEUTRAL, 0.0)
    assert (N.RISK_NEUTRAL, N.RISK_CVAR, N.RISK_WANG, N.RISK_CPW, N.RISK_POW) == (R.NEUTRAL, R.CVAR, R.WANG, R.CPW, R.POW)
    assert P.POLICIES == R.NAMES
    for text, want in [("cvar:0.25", (R.CVAR, 0.25)), ("cvar:1", (R.CVAR, 1.0)), ("cvar:1e-3", (R.CVAR, 1e-3)),
                       ("wang:-0.75", (R.WANG, -0.75)), ("wang:0", (R.WANG, 0.0)), ("wang:2.5", (R.WANG, 2.5)),
                       ("cpw:0.71", (R.CPW, 0.71)), ("cpw:1.0", (R.CPW, 1.0)), ("pow:-2", (R.POW, -2.0)),
                       ("pow:0", (R.POW, 0.0)), ("pow: 0.75", (R.POW, 0.75))]:
        assert P.parse(text) == want, text
        assert P.parse(P.canonical_id(want)) == want
    assert P.canonical_id(P.NEUTRAL) == "neutral"


@pytest.mark.parametrize("bad", ["cvar", "wang", "cpw:", "pow: ", "cvar:x", "cvar:0.1:2", "cvar:0", "cvar:1.5", "cvar:-0.1",
                                 "cpw:0", "cpw:1.5", "cvar:nan", "wang:nan", "cpw:nan", "pow:nan", "wang:inf", "pow:-inf",
                                 "norm:3", "CVaR:0.25", "", "neutral:1", 3, 0.25])
def test_parser_refuses(bad):
    from prism_amd.agents import risk_policies as P
    with pytest.raises(ValueError, match="iqn_risk_policy_id"):
        P.parse(bad)


def test_factory_refuses_before_a_model_is_built(monkeypatch):
    import prism_amd.config as config
    from prism_amd.factory import agent_factory, model_factory
    built = []
    monkeypatch.setattr(model_factory, "create_model", lambda *a, **k: built.append(a))

    def build(i, **over):
        return agent_factory.build_agent(config.baseline_config(i, device="cpu", **over), (10, 10, 4), 6)

    for bad in ("cvar", "cvar:0", "cvar:1.5", "cpw:nan", "sharpe:1"):
        with pytest.raises(ValueError, match="iqn_risk_policy_id"):
            build(2, iqn_risk_policy_id=bad)
    # Q heads: the IDS ensemble beside IQN, the DQN head alone, the DQN head beside IQN
    for i, over in ((3, {}), (0, {}), (2, dict(use_dqn=True))):
        with pytest.raises(ValueError, match="IQN-only"):
            build(i, iqn_risk_policy_id="cvar:0.25", **over)
    assert built == []
    # every preset is neutral: nothing changes for them
    presets = [config.DEFAULT_CONFIG, config.MINATAR_CONFIG, config.ADDITIVE_ABLATION_BASE_CONFIG,
               config.SUBTRACTIVE_ABLATION_BASE_CONFIG] + [config.baseline_config(i) for i in range(5)]
    assert all(c.iqn_risk_policy_id == "neutral" for c in presets)


def test_model_carries_the_policy_and_its_torch_forward_applies_it():
    """``IQNHead.forward(for_action=True)`` embeds beta(tau): with torch's generator rewound, the cvar:1 model gives the
    neutral model's values bit for bit (beta is the identity) and cvar:0.25 gives other values; the training-style forward
    (for_action=False) is the neutral one under every policy."""
    import contextlib
    import io
    import prism_amd.config as config
    from prism_amd.factory import model_factory
    models = {}
    for pid in ("neutral", "cvar:1", "cvar:0.25"):
        cfg = config.baseline_config(2, device="cpu", iqn_risk_policy_id=pid, iqn_quantile_samples_per_action=8)
        torch.manual_seed(5)
        with contextlib.redirect_stdout(io.StringIO()):
            models[pid] = model_factory.create_model((10, 10, 4), 6, cfg)
    assert models["neutral"].distribution_model.risk_policy is None
    assert models["cvar:0.25"].distribution_model.risk_policy == (R.CVAR, 0.25)
    obs = (torch.rand(3, 10, 10, 4) < 0.1).float()
    out = {}
    for pid, m in models.items():
        torch.manual_seed(9)
        out[pid] = m(obs)[1]
        torch.manual_seed(9)
        e = m.embedding_model(obs)
        out[pid, "train"] = m.distribution_model(e, n_quantile_samples=8)[0]
    assert torch.equal(out["neutral"], out["cvar:1"]) and not torch.equal(out["neutral"], out["cvar:0.25"])
    assert torch.equal(out["neutral", "train"], out["cvar:0.25", "train"])


@pytest.mark.parametrize("policy", [R.CVAR, R.WANG, R.CPW, R.POW])
def test_restatement_properties(policy):
    tau = _grid()
    assert tau[0] == 0.0 and tau[1] == np.float32(2.0 ** -24) and tau[-1] == np.float32(1.0 - 2.0 ** -24)
    for eta in ETAS[policy]:
        b = R.beta(policy, eta, tau)
        assert b.dtype == np.float32 and np.isfinite(b).all(), eta
        assert b[0] == 0.0 and not np.signbit(b[0]), f"beta(0) = {b[0]!r} at eta {eta}"
        assert float(b.min()) >= 0.0 and float(b.max()) <= 1.0, (eta, b.min(), b.max())
        if policy != R.CPW or eta > CPW_MONOTONE_FROM:
            assert (np.diff(b) >= 0).all(), f"policy {policy}, eta {eta}: not monotone"
    # the identities: to the last bit, cpw:1 within one float32 ulp
    ident = {R.CVAR: 1.0, R.WANG: 0.0, R.POW: 0.0}
    if policy in ident:
        np.testing.assert_array_equal(R.beta(policy, ident[policy], tau).view(np.uint32), tau.view(np.uint32))
    else:
        assert int(R.ulp_distance(R.beta(R.CPW, 1.0, tau), tau).max()) <= 1
        assert (np.diff(R.beta(R.CPW, 0.25, tau)) < 0).any(), "cpw below 0.279 dips: the bound above is the function's own"
    np.testing.assert_array_equal(R.beta(R.NEUTRAL, 0.0, tau).view(np.uint32), tau.view(np.uint32))


def test_restatement_directions():
    """cvar:eta and wang with eta < 0 put mass on the low quantiles (risk-averse), wang / pow with eta > 0 on the high."""
    tau = _grid()[1:]
    assert (R.beta(R.CVAR, 0.25, tau) <= tau).all() and (R.beta(R.WANG, -0.75, tau) <= tau).all()
    assert (R.beta(R.WANG, 0.75, tau) >= tau).all() and (R.beta(R.POW, 0.75, tau) >= tau).all()
    assert (R.beta(R.POW, -0.75, tau) <= tau).all()
    assert R.beta(R.CVAR, 0.25, np.float32([0.5]))[0] == np.float32(0.125)
    assert abs(float(R.beta64(R.WANG, -0.75, np.float32([0.5]))[0]) - 0.5 * math.erfc(0.75 / math.sqrt(2))) < 1e-15


@pytest.mark.parametrize("policy", [R.CVAR, R.WANG, R.CPW, R.POW])
def test_torch_form_equals_the_restatement(policy):
    """``risk_policies.distort`` (what ``IQNHead.forward`` applies): cvar bit for bit, the others within one float32 ulp
    (two float64 library evaluations, narrowed: they can differ only on a rounding boundary)."""
    from prism_amd.agents import risk_policies as P
    tau = _grid()
    for eta in ETAS[policy]:
        got = P.distort(torch.from_numpy(tau).view(-1, 1), (policy, eta))
        assert got.dtype == torch.float32 and tuple(got.shape) == (len(tau), 1)
        d = R.ulp_distance(got.numpy().reshape(-1), R.beta(policy, eta, tau))
        assert int(d.max()) <= (0 if policy == R.CVAR else 1), (policy, eta, int(d.max()))
    t = torch.from_numpy(tau)
    assert P.distort(t, P.NEUTRAL) is t


def _lib():
    import __graft_entry__ as g
    from prism_amd import _native as N
    if not os.path.exists(N.LIB_PATH):
        g.build()
    return N, N.lib()


def test_symbol_declared_exported_and_bound():
    import ctypes
    N, L = _lib()
    header = open(N.HEADER_PATH).read()
    assert "int prism_act_tau_distort(int32_t n, int32_t n_tau, int32_t policy, double eta, const float *tau_raw_in" in header
    for name, value in (("NEUTRAL", 0), ("CVAR", 1), ("WANG", 2), ("CPW", 3), ("POW", 4)):
        assert re.search(rf"#define PRISM_RISK_{name} {value}\b", header), name
        assert getattr(N, "RISK_" + name) == value
    assert hasattr(ctypes.CDLL(N.LIB_PATH), "prism_act_tau_distort")
    res, args = N.SIGNATURES["prism_act_tau_distort"]
    assert res is ctypes.c_int and len(args) == 11 and args[3] is ctypes.c_double and args[5] is args[6] is ctypes.c_uint64
    assert L.prism_act_tau_distort.argtypes == args
    assert L.prism_abi_version() == 3 and "#define PRISM_ABI_VERSION 3" in header


def test_argument_checks_without_device():
    N, L = _lib()
    p = 4096          # (a non-null address: every check fails before anything is launched or read)

    def call(n=4, T=8, policy=N.RISK_CVAR, eta=0.25, raw=None, word=None, out=p):
        return L.prism_act_tau_distort(n, T, policy, eta, raw, 1, 0, word, out, None, None)

    nan, inf = float("nan"), float("inf")
    refusals = [
        (dict(out=None), b"out_tau is null"),
        (dict(n=0), b"bad sizes"), (dict(n=-1), b"bad sizes"), (dict(T=0), b"bad sizes"), (dict(T=-8), b"bad sizes"),
        (dict(n=2 ** 14, T=2 ** 14), b"fewer than 2^28 samples"), (dict(n=2 ** 31 - 1, T=2 ** 31 - 1), b"fewer than 2^28 samples"),
        (dict(policy=-1), b"unknown policy"), (dict(policy=5), b"unknown policy"),
        (dict(eta=nan), b"eta is not finite"), (dict(eta=inf), b"eta is not finite"),
        (dict(policy=N.RISK_WANG, eta=nan), b"eta is not finite"), (dict(policy=N.RISK_WANG, eta=-inf), b"eta is not finite"),
        (dict(policy=N.RISK_POW, eta=inf), b"eta is not finite"), (dict(policy=N.RISK_CPW, eta=nan), b"eta is not finite"),
        (dict(policy=N.RISK_NEUTRAL, eta=nan), b"eta is not finite"),
        (dict(eta=0.0), b"eta outside (0, 1]"), (dict(eta=1.5), b"eta outside (0, 1]"), (dict(eta=-0.25), b"eta outside (0, 1]"),
        (dict(policy=N.RISK_CPW, eta=0.0), b"eta outside (0, 1]"), (dict(policy=N.RISK_CPW, eta=1.5), b"eta outside (0, 1]"),
        # (with raw samples and the word both given the word is ignored, not refused: the other checks still hold)
        (dict(raw=p, word=p, n=0), b"bad sizes"),
    ]
    for bad, text in refusals:
        assert call(**bad) == N.PRISM_ERR_INVALID, bad
        msg = L.prism_last_error()
        assert msg.startswith(b"prism_act_tau_distort: ") and text in msg, (bad, msg)


def test_the_kernel_has_no_private_segment(tmp_path):
    """Read from the code object's metadata of act_risk.hip: the private segment is 0 and the group segment is the 8 bytes
    through which a workgroup's ticket holder hands the count to the other lanes."""
    import shutil
    import subprocess
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    csrc = os.path.join(H.ROOT, "prism_amd", "csrc")
    out = tmp_path / "act_risk.s"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off",
                    "-I" + os.path.join(H.ROOT, "include"), "-I" + csrc, "-S", "--cuda-device-only", "-o", str(out),
                    os.path.join(csrc, "act_risk.hip")], check=True, timeout=600, stdout=subprocess.DEVNULL,
                   stderr=subprocess.DEVNULL)
    kernels = dict(re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", out.read_text(), re.S))
    names = [k for k in kernels if "tau_distort_kernel" in k]
    assert len(names) == 1
    assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", kernels[names[0]]).group(1)) == 0
    assert int(re.search(r"\.amdhsa_group_segment_fixed_size (\d+)", kernels[names[0]]).group(1)) == 8
