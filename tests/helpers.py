"""Shared test helpers: golden-fixture decoding and oracle construction."""
import contextlib
import glob
import io
import os

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")

UPDATE_CASES = ["iqn_small", "iqn_c3", "dqn_c2", "dqn_ln", "dqn_target_c2", "full_c4", "full_small",
                "full_notarget", "full_doubleq", "iqn_target", "iqn_doubleq", "iqn_tau32",
                # the reference's ablation presets and the stages its experiment files derive from them
                "abl_iqn", "abl_ln_notarget", "abl_doubleq", "abl_ids", "abl_ids_var", "abl_sub",
                # value squish of the TD target (loss_squish_fn_id): symlog / obs_look_further
                "iqn_symlog", "full_olf", "dqn_symlog"]

# away from the presets' scalars (tools/gen_golden.py CASES): Huber kappa 0.37 / 1.6, loss weights, Theil coefficient 0.5 on
# heads of unequal norm, propagate_grad off, clip thresholds below the gradient norm, other Adam hyper-parameters.  The
# centered-RMSprop one, dqn_rmsprop_scalars, is held where the RMSprop oracle lives (tests/test_optimizers.py NEW_CASES).
SCALAR_CASES = ["iqn_scalars", "iqn_t16_scalars", "iqn_l0_scalars", "full_scalars", "full_nodistgrad", "abl_scalars"]
UPDATE_CASES += SCALAR_CASES

# n-step chains recorded from the live reference (tools/gen_golden.py gen_nstep / NSTEP_CHAINS): whatever lies in the fixture
# directory, nstep_chain (n_step 3) first; tests/test_oracle_replay.py asserts which lengths and discounts they cover
NSTEP_CHAINS = sorted(os.path.basename(f)[:-4] for f in glob.glob(os.path.join(GOLDEN, "nstep_chain*.npz")))


def load_chain(name):
    return np.load(os.path.join(GOLDEN, f"{name}.npz"))


def load_case(name):
    return np.load(os.path.join(GOLDEN, f"update_{name}.npz"))


def case_overrides(g):
    return {str(k): eval(str(v), {}, {}) for k, v in zip(g["overrides_keys"], g["overrides_vals"])}


def case_config(g, device="cpu", **extra):
    from prism_amd import config as C
    base = {"minatar": C.MINATAR_CONFIG, "additive": C.ADDITIVE_ABLATION_BASE_CONFIG,
            "subtractive": C.SUBTRACTIVE_ABLATION_BASE_CONFIG}[str(g["base"]) if "base" in g else "minatar"]
    kw = dict(device=device, use_cuda_graph=False, use_e_greedy=False)
    kw.update(case_overrides(g))
    kw.update(extra)
    return C.derive(base, **kw)


def case_head_scale(g):
    """(a, b) of a fixture recorded with Q head h scaled by a + b * h after construction, or None."""
    return tuple(float(x) for x in g["head_scale"]) if "head_scale" in g.files else None


def scale_heads(named, head_scale):
    """Multiply every tensor of Q head h by a + b * h in place; `named`: (state_dict key, tensor) pairs.  None: nothing."""
    if head_scale is None:
        return
    a, b = head_scale
    with torch.no_grad():
        for k, v in named:
            if k.startswith("q_function_model.q_heads."):
                v.mul_(a + b * int(k.split(".")[2]))


def case_batch(g, step):
    B, C = int(g["B"]), int(g["C"])
    pre = f"s{step}/"
    n = B * 100 * C
    obs = np.unpackbits(g[pre + "obs_bits"])[:n].reshape(B, 10, 10, C).astype(np.float32)
    nobs = np.unpackbits(g[pre + "next_obs_bits"])[:n].reshape(B, 10, 10, C).astype(np.float32)
    batch = dict(obs=torch.from_numpy(obs), next_obs=torch.from_numpy(nobs),
                 reward=torch.from_numpy(g[pre + "reward"]).flatten(),
                 nonterminal=torch.from_numpy(g[pre + "nonterminal"]).flatten(),
                 gamma=torch.from_numpy(g[pre + "gamma"]).flatten(),
                 action=torch.from_numpy(g[pre + "action"]).flatten())
    w = torch.from_numpy(g[pre + "w"])
    taus = [torch.from_numpy(g[pre + f"tau{i}"]).reshape(-1, 1) for i in range(int(g[pre + "n_taus"]))]
    return batch, w, taus


def spec_from_config(cfg, C=4, A=6):
    from oracle.learner_ref import ModelSpec
    propagate = (cfg.ids_allow_distributional_gradients and cfg.use_ids) or not cfg.use_ids
    if cfg.use_ids:
        heads, hl, coef = cfg.ids_n_q_heads, cfg.ids_n_q_head_model_layers, cfg.ids_ensemble_variation_coef
    elif cfg.use_dqn:
        heads, hl, coef = 1, cfg.dqn_n_model_layers, 0.0
    else:
        heads, hl, coef = 0, 0, 0.0
    return ModelSpec(in_channels=C, n_actions=A, use_iqn=cfg.use_iqn, use_layer_norm=cfg.use_layer_norm,
                     n_basis=cfg.iqn_n_basis_elements, iqn_layers=cfg.iqn_quantile_model_layers,
                     n_tau=cfg.iqn_n_current_state_quantile_samples,
                     n_tau_next=cfg.iqn_n_next_state_quantile_samples, huber_k=cfg.iqn_huber_loss_kappa,
                     squish=str(cfg.loss_squish_fn_id),
                     dist_loss_weight=cfg.distributional_loss_weight, propagate_grad=propagate,
                     n_heads=heads, head_layers=hl, q_loss_weight=cfg.q_loss_weight, theil_coef=coef,
                     double_q=cfg.use_double_q_learning, max_grad_norm=cfg.max_grad_norm,
                     lr=cfg.learning_rate, beta1=cfg.adam_beta1, beta2=cfg.adam_beta2,
                     adam_eps=cfg.adam_epsilon)


def build_init_state(cfg, seed, C=4, A=6, head_scale=None):
    """Initial weights by construction (same seed, same layer creation order as the reference);
    returns (state_dict, target_state_dict or None).  `head_scale`: case_head_scale of the fixture."""
    from prism_amd.factory.model_factory import create_model
    torch.manual_seed(seed)
    with contextlib.redirect_stdout(io.StringIO()):
        m = create_model((10, 10, C), A, cfg)
        sd = {k: v.clone() for k, v in m.state_dict().items()}
        scale_heads(sd.items(), head_scale)
        tgt = None
        if cfg.use_target_network:
            create_model((10, 10, C), A, cfg)      # advances the RNG like agent_factory.py:15-18
            tgt = {k: v.clone() for k, v in sd.items()}
    return sd, tgt


def jitter_grads(sd, tgt, spec, batch, w, taus, seed, draws=6, ulps=2.4e-7):
    """The oracle's fp32 gradient at parameters jittered by about two units in the last place (`draws` times): where
    these disagree with the plain fp32 gradient, a ReLU unit sits within rounding distance of zero and two correct
    evaluations may differ by its whole contribution."""
    from oracle.learner_ref import LearnerOracle
    gen = torch.Generator().manual_seed(seed)
    out = []
    for _ in range(draws):
        jit = {k: v * (1.0 + ulps * torch.randn(v.shape, generator=gen)) for k, v in sd.items()}
        pj = LearnerOracle(jit, spec, tgt)
        pj.update(batch, w, taus, apply=False)
        out.append(pj.last["grads"])
    return out


def variant_config(device, over):
    """MinAtar preset as the parity tests on seeded random minibatches run it (tests/test_gpu_variants.py,
    tests/test_gpu_envelope.py): IQN alone with PER and LayerNorm unless `over` says otherwise."""
    from prism_amd.config import MINATAR_CONFIG, derive
    kw = dict(device=device, use_cuda_graph=False, use_e_greedy=False, use_ids=False, use_iqn=True, use_dqn=False,
              use_per=True, use_layer_norm=True)
    kw.update(over)
    return derive(MINATAR_CONFIG, **kw)


def random_batch(rng, B, C, A, cfg, mixed_gamma=False):
    """A seeded random minibatch, PER weights and the quantile samples of one update in the reference's draw order.
    `mixed_gamma`: a per-sample discount from {0.99, 0.99**2, 0.99**3} (n-step walks cut short), drawn last -- every other
    draw stays what it is without the keyword, which existing callers do not pass: their seeds were chosen on the one-gamma
    draw."""
    T, Tn = cfg.iqn_n_current_state_quantile_samples, cfg.iqn_n_next_state_quantile_samples
    batch = dict(obs=torch.from_numpy((rng.random((B, 10, 10, C)) < 0.15).astype(np.float32)),
                 next_obs=torch.from_numpy((rng.random((B, 10, 10, C)) < 0.15).astype(np.float32)),
                 reward=torch.from_numpy(rng.normal(0, 1, B).astype(np.float32)),
                 nonterminal=torch.from_numpy((rng.random(B) < 0.9).astype(np.float32)),
                 gamma=torch.from_numpy(np.full(B, 0.99 ** 3, np.float32)),
                 action=torch.from_numpy(rng.integers(0, A, B).astype(np.int64)))
    w = torch.from_numpy(rng.uniform(0.2, 1.0, B).astype(np.float32))
    n_next = 2 if (cfg.use_target_network and cfg.use_double_q_learning) else 1
    taus = [torch.from_numpy(rng.random((B * T, 1)).astype(np.float32))]
    taus += [torch.from_numpy(rng.random((B * Tn, 1)).astype(np.float32)) for _ in range(n_next)]
    if mixed_gamma:
        batch["gamma"] = torch.from_numpy((0.99 ** rng.integers(1, 4, B)).astype(np.float32))
    return batch, w, taus


def checksums(sd):
    s = np.array([float(v.double().sum()) for v in sd.values()])
    l2 = np.array([float(v.double().norm()) for v in sd.values()])
    return s, l2


def case_act(g):
    """Acting inputs / the reference's outputs of an update fixture: (obs (n,10,10,C), taus (T*n,1) or None, dict)."""
    n, C = int(g["act/n"]), int(g["C"])
    obs = np.unpackbits(g["act/obs_bits"])[:n * 100 * C].reshape(n, 10, 10, C).astype(np.float32)
    taus = torch.from_numpy(g["act/tau"]).reshape(-1, 1) if "act/tau" in g.files else None
    return torch.from_numpy(obs), taus, {k[4:]: g[k] for k in g.files if k.startswith("act/")}


# ---- Philox4x32-10 on the host (Salmon et al., SC'11) -- restates prism_amd/csrc/common.h::Philox so that a test can
# re-draw what a kernel drew on the device (PER masses, quantile samples) from (seed, counter, stream key)
def philox4x32(seed, ctr, stream):
    """ctr: uint64 array of counters; returns uint32 array [n, 4]."""
    ctr = np.asarray(ctr, dtype=np.uint64)
    m32 = np.uint64(0xFFFFFFFF)
    c0, c1 = ctr & m32, ctr >> np.uint64(32)
    c2 = np.full_like(ctr, np.uint64(stream) & m32)
    c3 = np.full_like(ctr, np.uint64(stream) >> np.uint64(32))
    a, b = np.uint64(seed & 0xFFFFFFFF), np.uint64((seed >> 32) & 0xFFFFFFFF)
    for _ in range(10):
        p0, p1 = np.uint64(0xD2511F53) * c0, np.uint64(0xCD9E8D57) * c2
        h0, l0, h1, l1 = p0 >> np.uint64(32), p0 & m32, p1 >> np.uint64(32), p1 & m32
        c0, c1, c2, c3 = h1 ^ c1 ^ a, l1, h0 ^ c3 ^ b, l0
        a = (a + np.uint64(0x9E3779B9)) & m32
        b = (b + np.uint64(0xBB67AE85)) & m32
    return np.stack([c0, c1, c2, c3], axis=1).astype(np.uint32)


TAU_KEY = 0x54415530          # "TAU0": the quantile-sample streams are keyed TAU_KEY + stream id
TAU_CUR, TAU_NEXT_ONLINE, TAU_NEXT_TARGET, TAU_ACT = 0, 1, 2, 3


def u32_to_unit_float(x):
    """common.h::u32_to_unit_float: the top 24 bits of a word as a float32 in [0, 1) (every step exact in float32)."""
    return (np.asarray(x, dtype=np.uint32) >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)


def philox_taus(seed, offset, T, B, sid):
    """The IQN quantile samples every drawing site must produce (step_kernels.h cos_basis_block, fwd_kernels.h both tile
    prologues): float32[T * B], tau-major as the reference's ``torch.rand([T * B, 1])`` is read (iqn_model.py:66-68),

        tau[t * B + b] = float32(Philox(seed, offset + t * B + b, TAU_KEY + sid)[0] >> 8) * 2**-24

    sid: 0 current state, 1 next state on the online network, 2 next state on the target network, 3 acting."""
    r = philox4x32(seed, np.uint64(offset) + np.arange(int(T) * int(B), dtype=np.uint64), TAU_KEY + int(sid))
    return u32_to_unit_float(r[:, 0])


def tau_streams(cfg):
    """Stream ids an update of this configuration draws, in the order ``taus`` lists them for the oracle
    (learner.hip fill_iqn_args; iqn_model.py:104,112-126)."""
    if not cfg.use_iqn:
        return []
    sids = [TAU_CUR]
    if not cfg.use_target_network or cfg.use_double_q_learning:
        sids.append(TAU_NEXT_ONLINE)
    if cfg.use_target_network:
        sids.append(TAU_NEXT_TARGET)
    return sids


def tau_span(cfg, B):
    """Counters one update consumes of the learner's one counter space, whichever path ran it (hip_agent.py update /
    step_fused): three streams' worth of max(T, T') * B, whether or not the configuration draws all three."""
    return 3 * max(cfg.iqn_n_current_state_quantile_samples, cfg.iqn_n_next_state_quantile_samples) * int(B)


def philox_per_mass(seed, offset, batch, p_sum):
    """The masses step_front_kernel / per_sample_kernel draw: U(0, p_sum) in float64 (53 random bits, as numpy's
    random_sample), narrowed to fp32 (replay_kernels.h, key "PERM")."""
    r = philox4x32(seed, np.uint64(offset) + np.arange(batch, dtype=np.uint64), 0x5045524D)
    a, b = (r[:, 0] >> np.uint32(5)).astype(np.float64), (r[:, 1] >> np.uint32(6)).astype(np.float64)
    u = (a * 67108864.0 + b) / 9007199254740992.0
    return (0.0 + (np.float64(np.float32(p_sum)) - 0.0) * u).astype(np.float32)


def philox_uniform_index(seed, offset, batch, size):
    """The slots uniform_sample_kernel / step_front_kernel draw for uniform replay (torchrl RandomSampler,
    exp_buffer_factory.py:30-33): floor(x * size / 2**64) of a 64-bit Philox word, key "UNIF"."""
    r = philox4x32(seed, np.uint64(offset) + np.arange(batch, dtype=np.uint64), 0x554E4946)
    return np.array([((int(a) << 32 | int(b)) * int(size)) >> 64 for a, b in zip(r[:, 0], r[:, 1])], dtype=np.int64)


# ---- the replay half of one fused step against the oracle (tests/test_gpu_fullsize_parity.py, tests/test_gpu_replay_geometry.py)
def oracle_ring(buf, cfg):
    """ReplayOracle over the device ring's small arrays; observation rows are filled lazily (calloc'ed, only the sampled
    slots' pages ever become resident: the 1.25 M-slot ring would be 4 GB of host memory otherwise)."""
    from oracle import per_ref
    orc = per_ref.ReplayOracle(buf.capacity, buf.obs_elems, cfg.n_step_returns_length, cfg.gamma, cfg.per_alpha,
                               buf.buffer._sampler._beta)          # (the beta the sampling launches read)
    orc.reward[:] = buf.reward.cpu().numpy()
    orc.action[:] = buf.action.cpu().numpy()
    orc.flags[:] = buf.flags.cpu().numpy()
    orc.link[:] = buf.link.cpu().numpy()
    orc.length = buf._size
    assert orc.sampler.sum_tree.capacity == buf.tree_capacity
    return orc


def fill_rows(orc, buf, idx):
    """Observation rows the n-step walk of `idx` can touch: the slots themselves and <= n_step - 1 hops of links."""
    slots, cur = [idx], idx
    for _ in range(orc.n_step - 1):
        nxt = orc.link[cur]
        cur = np.where(nxt >= 0, nxt, cur)
        slots.append(cur)
    s = np.unique(np.concatenate(slots))
    st = torch.from_numpy(s).to(buf.device)
    orc.obs[s] = buf.obs[st].cpu().numpy()
    orc.succ_obs[s] = buf.succ_obs[st].cpu().numpy()


def replay_snapshot(buf, agent):
    """Before a fused step: both priority trees, the running maximum and the Philox counters the step's draws start at."""
    snap = dict(per_ctr=int(agent.rng_counters[0].item()) if agent._B is not None else 0, draws0=buf._draws)
    if buf.use_per:
        snap.update(sum0=buf.sum_tree.cpu().numpy().copy(), min0=buf.min_tree.cpu().numpy().copy(),
                    max0=float(buf.per_state[0].item()))
    return snap


def check_replay_front(buf, orc_ring, snap, B, step, fill=True):
    """After the step: same trees, same masses -> same slots and IS weights; then the n-step walk + collate of those slots.
    Returns (slots, the oracle's IS weights, the oracle's batch).  `fill`: the oracle's observation rows are filled lazily
    from the device ring (oracle_ring)."""
    smp = orc_ring.sampler
    idx = buf._index.cpu().numpy()
    sum0, min0, max0, per_ctr, draws0 = (snap.get(k) for k in ("sum0", "min0", "max0", "per_ctr", "draws0"))
    if buf.use_per:
        smp.sum_tree.values()[:] = sum0
        smp.min_tree.values()[:] = min0
        smp.max_priority = max0
        p_sum = smp.sum_tree.query(0, buf._size)
        mass = philox_per_mass(buf.seed, draws0 + per_ctr, B, p_sum)
        idx_o, w_o, ps_o, pm_o = smp.sample(buf._size, mass)
        np.testing.assert_array_equal(idx, idx_o, err_msg=f"step {step}: sampled slots")
        np.testing.assert_array_equal(buf._weight.cpu().numpy(), w_o, err_msg=f"step {step}: IS weights")
        assert np.float32(ps_o) == np.float32(buf.per_state[1].item()) and np.float32(pm_o) == np.float32(buf.per_state[2].item())
    else:
        # uniform replay (configs[0]; exp_buffer_factory.py:30-33): slot = floor(u * size) of the same Philox word, IS weight 1
        idx_o = philox_uniform_index(buf.seed, draws0 + per_ctr, B, buf._size)
        np.testing.assert_array_equal(idx, idx_o, err_msg=f"step {step}: uniformly sampled slots")
        w_o = np.ones(B, dtype=np.float32)
    # ---- n-step walk + collate
    if fill:
        fill_rows(orc_ring, buf, idx)
    g = orc_ring.gather(idx)
    np.testing.assert_array_equal(buf._obs.cpu().numpy().reshape(B, -1), g["obs"])
    np.testing.assert_array_equal(buf._next_obs.cpu().numpy().reshape(B, -1), g["next_obs"])
    np.testing.assert_array_equal(buf._reward.cpu().numpy().ravel(), g["reward"])
    np.testing.assert_array_equal(buf._gamma.cpu().numpy().ravel(), g["gamma"])
    np.testing.assert_array_equal(buf._nonterminal.cpu().numpy().ravel().astype(np.uint8), g["nonterminal"])
    np.testing.assert_array_equal(buf._action.cpu().numpy().ravel(), g["action"])
    return idx, w_o, g


def check_replay_writeback(buf, smp, idx, td_abs, step):
    """The oracle's update_priority fed the device's own |td|: EVERY node of both trees, duplicates included, and the
    running maximum.  Uniform replay has nothing to write back."""
    if not buf.use_per:
        return
    smp.update_priority(idx, td_abs)
    np.testing.assert_array_equal(buf.sum_tree.cpu().numpy(), smp.sum_tree.values(), err_msg=f"step {step}: sum tree")
    np.testing.assert_array_equal(buf.min_tree.cpu().numpy(), smp.min_tree.values(), err_msg=f"step {step}: min tree")
    assert np.float32(smp.max_priority) == np.float32(buf.per_state[0].item())
