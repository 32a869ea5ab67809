"""No GPU needed: the optimizer choice beside Adam -- centered RMSprop and SGD (the reference's
agent_factory.py:40-58) -- on the host side: the factory's three-way choice, torch-format optimizer state, the committed
reference checkpoint, the two new entry points' argument checks, and the emitted gfx950 kernels."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import helpers as H

NEW_CASES = ["dqn_c2_rmsprop", "iqn_c3_rmsprop", "abl_ln_notarget_rmsprop", "full_small_sgd",
             # centered RMSprop away from the preset: alpha 0.9, eps 0.02, lr 5e-4, q_loss_weight 0.4, clip at 0.5
             "dqn_rmsprop_scalars"]


def swap_optimizer(orc, cfg):
    """The oracle with the optimizer the reference builds for this configuration (``LearnerOracle.opt`` is public)."""
    params = list(orc.p.values())
    if cfg.use_adam:
        return orc
    if cfg.use_rmsprop:
        orc.opt = torch.optim.RMSprop(params, lr=cfg.learning_rate, alpha=cfg.rmsprop_alpha, eps=cfg.rmsprop_epsilon,
                                      centered=True)
    else:
        orc.opt = torch.optim.SGD(params, lr=cfg.learning_rate)
    return orc


def named_params(seed=0):
    gen = torch.Generator().manual_seed(seed)
    shapes = [("a.weight", (16, 4, 3, 3)), ("a.bias", (16,)), ("b.weight", (6, 5)), ("b.bias", (3,))]      # 629 floats: not a multiple of 4
    return [(n, torch.randn(s, generator=gen)) for n, s in shapes]


def flat_of(named):
    return torch.cat([p.reshape(-1) for _, p in named]).clone()


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from prism_amd import _native as N
    if not os.path.exists(N.LIB_PATH):
        g.build()
    return N.lib()


# ---------------------------------------------------------------------------------------------- factory
@pytest.mark.parametrize("use_adam,use_rmsprop,expect", [(True, False, "HipAdam"), (True, True, "HipAdam"),
                                                         (False, True, "HipRMSprop"), (False, False, "HipSGD")])
def test_factory_choice_follows_the_reference_precedence(use_adam, use_rmsprop, expect):
    from prism_amd import config as C
    from prism_amd.agents import hip_agent
    from prism_amd.factory import model_factory
    cfg = C.derive(C.MINATAR_CONFIG, use_adam=use_adam, use_rmsprop=use_rmsprop)
    model_factory.check_supported(cfg)          # no optimizer is refused any more
    named = named_params()
    opt = hip_agent.build_optimizer(cfg, named, flat_of(named))
    assert type(opt).__name__ == expect
    g = opt.param_groups[0]
    assert g["lr"] == cfg.learning_rate and g["params"] == [0, 1, 2, 3]
    if expect == "HipRMSprop":
        assert (g["alpha"], g["eps"], g["centered"], g["momentum"], g["weight_decay"]) == \
            (cfg.rmsprop_alpha, cfg.rmsprop_epsilon, True, 0, 0)
        h = opt.native_hyper()
        assert (h.kind, h.lr, h.alpha, h.eps) == (1, cfg.learning_rate, cfg.rmsprop_alpha, cfg.rmsprop_epsilon)
    if expect == "HipSGD":
        assert g["momentum"] == 0 and g["weight_decay"] == 0 and not g["nesterov"]
        assert opt.native_hyper().kind == 2
    if expect == "HipAdam":
        assert opt.native_hyper() is None and g["betas"] == (cfg.adam_beta1, cfg.adam_beta2)


def test_agent_factory_no_longer_refuses_other_optimizers():
    """Without a device the agent itself cannot be built; the refusal that used to come first must be gone."""
    from prism_amd import config as C
    from prism_amd._native import NativeLibraryError
    from prism_amd.factory import agent_factory
    import contextlib
    import io
    cfg = C.derive(C.MINATAR_CONFIG, use_adam=False, use_rmsprop=True, device="cpu", use_ids=False, use_iqn=False,
                   use_dqn=True, use_layer_norm=False)
    with contextlib.redirect_stdout(io.StringIO()), pytest.raises(NativeLibraryError):
        agent_factory.build_agent(cfg, (10, 10, 4), 6)


# ---------------------------------------------------------------------------------------------- state format
def torch_optimizer(kind, params):
    if kind == "rmsprop":
        return torch.optim.RMSprop(params, lr=2.5e-4, alpha=0.95, eps=0.01, centered=True)
    if kind == "sgd":
        return torch.optim.SGD(params, lr=2.5e-4)
    return torch.optim.Adam(params, lr=2.5e-4, betas=(0.9, 0.999), eps=1.5e-4)


def hip_optimizer(kind, named):
    from prism_amd.agents import hip_agent as A
    flat = flat_of(named)
    if kind == "rmsprop":
        return A.HipRMSprop(named, flat, 2.5e-4, 0.95, 0.01)
    if kind == "sgd":
        return A.HipSGD(named, flat, 2.5e-4)
    return A.HipAdam(named, flat, 2.5e-4, (0.9, 0.999), 1.5e-4)


@pytest.mark.parametrize("kind", ["adam", "rmsprop", "sgd"])
def test_state_dict_interchanges_with_torch_optim(kind):
    named = named_params()
    # torch's own state after three real steps ...
    params = [p.clone().requires_grad_(True) for _, p in named]
    topt = torch_optimizer(kind, params)
    gen = torch.Generator().manual_seed(5)
    for _ in range(3):
        for p in params:
            p.grad = torch.randn(p.shape, generator=gen)
        topt.step()
    tsd = topt.state_dict()
    # ... loads into the host optimizer, whose own state_dict has torch's keys and values ...
    hopt = hip_optimizer(kind, named)
    if kind == "adam":          # (Adam's files stay what they were: the key set of the torch release they were written for)
        assert set(hopt.param_groups[0]) <= set(tsd["param_groups"][0])
    else:
        assert set(hopt.param_groups[0]) == set(tsd["param_groups"][0])
    hopt.load_state_dict(tsd)
    hsd = hopt.state_dict()
    assert all(tsd["param_groups"][0][k] == v for k, v in hsd["param_groups"][0].items())
    assert set(hsd["state"]) == set(tsd["state"])
    for i, st in tsd["state"].items():
        assert list(hsd["state"][i]) == list(st)
        for k, v in st.items():
            assert torch.equal(hsd["state"][i][k], v) if torch.is_tensor(v) else hsd["state"][i][k] == v, (i, k)
    if kind != "sgd":
        assert int(hopt.step_t.item()) == 3
    # ... and loads back into a fresh torch optimizer without loss (what the reference's Agent.load does with the file)
    params2 = [p.clone().requires_grad_(True) for _, p in named]
    topt2 = torch_optimizer(kind, params2)
    topt2.load_state_dict(hsd)
    back = topt2.state_dict()
    assert all(back["param_groups"][0][k] == v for k, v in tsd["param_groups"][0].items())
    for i, st in tsd["state"].items():
        for k, v in st.items():
            assert torch.equal(back["state"][i][k], v) if torch.is_tensor(v) else back["state"][i][k] == v
    # a fresh optimizer writes what a fresh torch optimizer writes: no per-parameter state
    assert hip_optimizer(kind, named).state_dict()["state"] == torch_optimizer(kind, params2).state_dict()["state"] == {}


def test_other_rmsprop_and_sgd_forms_are_refused_on_load():
    named = named_params()
    params = [p.clone().requires_grad_(True) for _, p in named]
    with pytest.raises(ValueError):
        hip_optimizer("rmsprop", named).load_state_dict(torch.optim.RMSprop(params, lr=1e-3).state_dict())      # not centered
    with pytest.raises(ValueError):
        hip_optimizer("sgd", named).load_state_dict(torch.optim.SGD(params, lr=1e-3, momentum=0.9).state_dict())


def test_committed_rmsprop_checkpoint_has_the_expected_sums():
    ck = os.path.join(H.GOLDEN, "ref_checkpoint_rmsprop", "agent")
    exp = np.load(os.path.join(H.GOLDEN, "ref_checkpoint_rmsprop_expected.npz"))
    sd = torch.load(os.path.join(ck, "optimizer.pt"), map_location="cpu", weights_only=True)
    model = torch.load(os.path.join(ck, "model.pt"), map_location="cpu", weights_only=True)
    assert list(model.keys()) == [str(n) for n in exp["param_names"]]
    np.testing.assert_array_equal(np.array([float(v.double().sum()) for v in model.values()]), exp["sum"])
    g = sd["param_groups"][0]
    assert sorted(k for k in g if k != "params") == [str(k) for k in exp["group_keys"]]
    assert (g["lr"], g["alpha"], g["eps"], g["centered"]) == (float(exp["lr"]), float(exp["alpha"]), float(exp["eps"]), True)
    n = len(model)
    assert sorted(sd["state"]) == list(range(n))
    for i in range(n):
        st = sd["state"][i]
        assert float(st["step"]) == float(exp["step"]) == 2.0
        assert float(st["square_avg"].double().sum()) == float(exp["square_avg_sum"][i])
        assert float(st["grad_avg"].double().sum()) == float(exp["grad_avg_sum"][i])
    # the host optimizer takes it whole
    from prism_amd.agents import hip_agent as A
    named = list(model.items())
    hopt = A.HipRMSprop(named, flat_of(named), 1.0, 0.5, 0.5)
    hopt.load_state_dict(sd)
    assert int(hopt.step_t.item()) == 2 and hopt.native_hyper().lr == float(exp["lr"])
    assert abs(float(hopt.square_avg.double().sum()) - float(exp["square_avg_sum"].sum())) < 1e-9
    assert abs(float(hopt.grad_avg.double().sum()) - float(exp["grad_avg_sum"].sum())) < 1e-9


# ---------------------------------------------------------------------------------------------- fixtures vs oracle
@pytest.mark.parametrize("name", NEW_CASES)
def test_oracle_with_swapped_optimizer_reproduces_the_reference(name):
    """The new fixtures against the torch-CPU oracle with ``opt`` swapped: same losses and same parameters after every
    step as the live reference recorded.  At width 128 the oracle's own fp32 and fp64 gradients agree within the
    gradient tolerance of the GPU parity test (1e-4 max|g| + 1e-7): those cases need no kink allowance."""
    from oracle.learner_ref import LearnerOracle
    g = H.load_case(name)
    cfg = H.case_config(g)
    assert not cfg.use_adam
    sd, tgt = H.build_init_state(cfg, int(g["seed"]), C=int(g["C"]), A=int(g["A"]), head_scale=H.case_head_scale(g))
    orc = swap_optimizer(LearnerOracle(sd, H.spec_from_config(cfg, C=int(g["C"]), A=int(g["A"])), tgt), cfg)
    width = max(cfg.iqn_quantile_model_feature_dim if cfg.use_iqn else 0, cfg.ids_q_head_feature_dim if cfg.use_ids else 0)
    for step in range(int(g["steps"])):
        batch, w, taus = H.case_batch(g, step)
        g64 = orc.grads_fp64(batch, w, taus) if width <= 128 else None
        td = orc.update(batch, w, taus)
        pre = f"s{step}/"
        np.testing.assert_allclose(td.numpy(), g[pre + "td"], rtol=0, atol=1e-5)
        assert abs(float(orc.last["total"]) - float(g[pre + "total"])) < 1e-5
        if g64 is not None:
            for k, go in orc.last["grads"].items():
                err = float((go.double() - g64[k]).abs().max())
                assert err <= 1e-4 * float(go.abs().max()) + 1e-7, f"step {step} {k}: fp32/fp64 gradients differ by {err:.3e}"
        s, l2 = H.checksums(orc.state_dict())
        np.testing.assert_allclose(l2, g[pre + "post_l2"], rtol=2e-6, atol=1e-7)
        assert (np.abs(s - g[pre + "post_sum"]) <= 2e-6 * np.array([v.numel() for v in sd.values()])).all()
        if cfg.use_target_network and step == 0:
            orc.sync_target()


# ---------------------------------------------------------------------------------------------- C ABI
def _supported_desc(N):
    d = N.LearnerDesc()
    dm = d.dims
    dm.in_channels, dm.n_actions, dm.embed_dim, dm.use_iqn = 4, 6, 1024, 1
    dm.n_basis, dm.iqn_layers, dm.iqn_width, dm.n_tau, dm.n_tau_next, dm.use_layer_norm = 64, 1, 128, 8, 8, 1
    d.batch = 256
    return d


def test_new_entry_points_are_exported_and_check_their_arguments(lib):
    from prism_amd import _native as N
    raw = ctypes.CDLL(N.LIB_PATH)
    for name in ("prism_learner_clip_step", "prism_step_back_opt"):
        assert hasattr(raw, name) and name in N.SIGNATURES
    assert (N.OPT_ADAM, N.OPT_RMSPROP, N.OPT_SGD) == (0, 1, 2)
    assert ctypes.sizeof(N.OptHyper) == 8 + 3 * 8          # int32 kind (+ padding), three doubles
    hdr = open(N.HEADER_PATH).read()
    for k, v in (("ADAM", 0), ("RMSPROP", 1), ("SGD", 2)):
        assert re.search(r"#define PRISM_OPT_%s %d\b" % (k, v), hdr)
    d, rp = _supported_desc(N), N.ReplayDesc()
    opt = N.OptHyper(N.OPT_RMSPROP, 2.5e-4, 0.95, 0.01)
    # null descriptor / null hyper-parameters / unknown kind: PRISM_ERR_INVALID
    assert lib.prism_learner_clip_step(None, ctypes.byref(opt), None) == N.PRISM_ERR_INVALID
    assert b"null descriptor" in lib.prism_last_error()
    assert lib.prism_learner_clip_step(ctypes.byref(d), None, None) == N.PRISM_ERR_INVALID
    assert b"null optimizer" in lib.prism_last_error()
    assert lib.prism_step_back_opt(None, ctypes.byref(opt), ctypes.byref(rp), None, 0.5, 1e-6, None) == N.PRISM_ERR_INVALID
    assert lib.prism_step_back_opt(ctypes.byref(d), None, ctypes.byref(rp), None, 0.5, 1e-6, None) == N.PRISM_ERR_INVALID
    assert lib.prism_learner_clip_step(ctypes.byref(d), ctypes.byref(N.OptHyper(7, 1e-3, 0.0, 0.0)), None) == N.PRISM_ERR_INVALID
    assert b"optimizer kind" in lib.prism_last_error()
    # the fused tail is Adam's: refused for the other kinds, never run as Adam
    d.fuse_tail = 1
    for kind in (N.OPT_RMSPROP, N.OPT_SGD):
        o = N.OptHyper(kind, 2.5e-4, 0.95, 0.01)
        assert lib.prism_learner_clip_step(ctypes.byref(d), ctypes.byref(o), None) == N.PRISM_ERR_UNSUPPORTED
        assert b"fused tail" in lib.prism_last_error()
        assert lib.prism_step_back_opt(ctypes.byref(d), ctypes.byref(o), ctypes.byref(rp), None, 0.5, 1e-6, None) == \
            N.PRISM_ERR_UNSUPPORTED
    # with the tail off the call goes on to the shared descriptor checks (null buffers here), as prism_learner_clip_adam does
    d.fuse_tail = 0
    assert lib.prism_learner_clip_step(ctypes.byref(d), ctypes.byref(opt), None) == N.PRISM_ERR_INVALID
    assert b"null parameter buffers" in lib.prism_last_error()
    assert lib.prism_learner_clip_adam(ctypes.byref(d), None) == N.PRISM_ERR_INVALID


# ---------------------------------------------------------------------------------------------- emitted kernels
@pytest.fixture(scope="module")
def optimizer_isa(tmp_path_factory):
    """gfx950 assembly of learner.hip (Adam's kernels) and opt_step.hip (the other kinds), compiled as tests/test_abi.py
    compiles its translation units: {source name: text}."""
    import shutil
    import subprocess
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    csrc = os.path.join(H.ROOT, "prism_amd", "csrc")
    tmp = tmp_path_factory.mktemp("isa_opt")
    out = {}
    for src in ("learner.hip", "opt_step.hip"):
        o = tmp / (src + ".s")
        subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off",
                        "-I" + os.path.join(H.ROOT, "include"), "-I" + csrc, "-S", "--cuda-device-only",
                        "-o", str(o), os.path.join(csrc, src)], check=True, timeout=900,
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        out[src] = o.read_text()
    return out


def _resource_blocks(text):
    out = {}
    for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, re.S):
        out[m.group(1)] = {k: int(v) for k, v in re.findall(r"\.amdhsa_(\w+) (\d+)\s", m.group(2))}
    return out


def test_new_kernels_exist_and_adams_keep_their_resource_block(optimizer_isa):
    blocks = _resource_blocks(optimizer_isa["opt_step.hip"])
    new = [k for k in blocks if "clip_opt_kernel" in k or "step_back_opt_kernel" in k]
    # one instantiation per kind (ILi1E = RMSprop, ILi2E = SGD) of each of the two launches, none for Adam (ILi0E)
    assert sorted(re.search(r"(clip_opt_kernel|step_back_opt_kernel)ILi(\d)E", k).groups() for k in new) == \
        [("clip_opt_kernel", "1"), ("clip_opt_kernel", "2"), ("step_back_opt_kernel", "1"), ("step_back_opt_kernel", "2")]
    text = optimizer_isa["opt_step.hip"]
    for k in new:
        assert blocks[k]["private_segment_fixed_size"] == 0, k          # no scratch ...
        body = text[text.find("\n" + k + ":"):text.find(".amdhsa_kernel " + k)]
        assert len(body) > 1000 and not re.search(r"scratch_(load|store)", body), k
        # ... and the step counter's ticket sits behind a workgroup barrier, as in Adam's block
        assert re.search(r"s_barrier(.|\n)*global_atomic_add", body), k
    # SGD streams no state: fewer registers than the RMSprop form
    clip = {re.search(r"ILi(\d)E", k).group(1): blocks[k] for k in new if "clip_opt_kernel" in k}
    assert clip["2"]["next_free_vgpr"] < clip["1"]["next_free_vgpr"]
    # the translation unit with every kernel of the Adam step holds none of the new ones (its code object is the one it
    # was), and Adam's two kernels have the resource block they had before the optimizer kind became a template parameter
    blocks = _resource_blocks(optimizer_isa["learner.hip"])
    assert not [k for k in blocks if "clip_opt_kernel" in k or "step_back_opt_kernel" in k]
    adam = {k: v for k, v in blocks.items() if re.search(r"\d+(clip_adam_kernel|step_back_kernel)E", k)}
    assert len(adam) == 2
    want = {"clip_adam_kernel": dict(group_segment_fixed_size=1040, private_segment_fixed_size=0, kernarg_size=384,
                                     next_free_vgpr=73, next_free_sgpr=100, accum_offset=76),
            "step_back_kernel": dict(group_segment_fixed_size=23696, private_segment_fixed_size=0, kernarg_size=704,
                                     next_free_vgpr=113, next_free_sgpr=100, accum_offset=116)}
    for k, v in adam.items():
        w = want["clip_adam_kernel" if "clip_adam_kernel" in k else "step_back_kernel"]
        assert {f: v[f] for f in w} == w, k
