#!/usr/bin/env python3
"""Generate tests/golden/*.npz by RUNNING the reference (imported from /root/reference).

Build-container only: the reference does not exist on the GPU box, and nothing in tests/ or the
product imports it.  The fixtures hold DATA only — seeds, inputs, captured quantile samples and the
reference's outputs — never reference source.

    python tools/gen_golden.py            # writes tests/golden/{update_*,nstep_*}.npz

What is captured:
  update_<case>.npz  Agent.update() (non-graph path, prism/agents/agent.py:53-79) for N steps on
                     seeded synthetic MinAtar-shaped batches: inputs, taus (torch.rand patched to
                     record, order current -> next -> [target]), per-sample losses / td errors,
                     total loss, per-tensor grad L2 norms, global grad norm, per-tensor parameter
                     checksums after every step (+ full tensors for the small cases).
  nstep_chain.npz    TimestepBuffer._compute_n_step / _timesteps_to_batch
                     (prism/experience/timestep_buffer.py:79-238) on hand-built Timestep chains.
  nstep_chain_*.npz  the same at n_step 1, 2, 5 and 15 and other discounts (NSTEP_CHAINS); written by
                     `python tools/gen_golden.py nstep_more`, which never touches nstep_chain.npz.
  collector_bookkeeping.npz  reward clip, episodic reward and training-reward EMA of the reference's collector
                     (collector_process_interface.py:129-139, experience_collector.py:113-118), per timestep;
                     `python tools/gen_golden.py collector`.
  evaluator_runs.npz SyncAgentEvaluator.evaluate_agent (prism/evals/sync_agent_evaluator.py:25-62) over scripted
                     single-environment runs: rewards, end kinds, horizon, the returned ep_rews as float64 bits and the
                     timesteps consumed; `python tools/gen_golden.py evaluator`.
"""
import contextlib
import io
import os
import sys
import types

import numpy as np
import torch

REF = "/root/reference"
OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden")
sys.dont_write_bytecode = True


def _import_reference():
    sys.path.insert(0, REF)
    # stand-ins for absent third-party modules the experience half imports at module scope
    td = types.ModuleType("tensordict")

    class TensorDict(dict):
        def __init__(self, d=None, batch_size=None, device=None):
            super().__init__(d or {})
            self.batch_size, self.device = batch_size, device

    td.TensorDict = TensorDict
    sys.modules["tensordict"] = td
    sys.modules["wandb"] = types.ModuleType("wandb")


def synth_batch(rng, B, C=4, A=6, p_term=0.05, p_short=0.05):
    """p_short: share of samples whose n-step walk was cut short (gamma 0.99**2, half of them 0.99)."""
    obs = (rng.random((B, 1, 10, 10, C)) < 0.1).astype(np.float32)
    nobs = (rng.random((B, 1, 10, 10, C)) < 0.1).astype(np.float32)
    rew = rng.standard_normal((B, 1)).astype(np.float32)
    nonterm = rng.random((B, 1)) >= p_term
    g = np.full((B, 1), 0.99 ** 3, np.float32)
    sel = rng.random(B)
    g[sel < p_short, 0] = np.float32(0.99 ** 2)
    g[sel < p_short / 2, 0] = np.float32(0.99)
    act = rng.integers(0, A, size=(B, 1)).astype(np.int64)
    w = (rng.random(B).astype(np.float32) * 0.9 + 0.1)
    return dict(obs=obs, next_obs=nobs, reward=rew, nonterminal=nonterm, gamma=g, action=act, w=w)


def to_ref_batch(b):
    t = torch.from_numpy
    return {"observation": t(b["obs"]), "next": {"observation": t(b["next_obs"]), "reward": t(b["reward"])},
            "nonterminal": t(b["nonterminal"]), "gamma": t(b["gamma"]), "action": t(b["action"])}


def tensor_stats(sd):
    names = list(sd.keys())
    s = np.array([float(sd[k].double().sum()) for k in names])
    l2 = np.array([float(sd[k].double().norm()) for k in names])
    return names, s, l2


_ADAM_SCALARS = dict(learning_rate=5e-4, adam_beta1=0.8, adam_beta2=0.95, adam_epsilon=3e-4)
_MIXED = (0.3, 0.5)

CASES = {
    # name: (config overrides, B, steps, store_full_params[, (p_term, p_short)])
    "iqn_small": (dict(use_ids=False, use_iqn=True, use_dqn=False, iqn_n_current_state_quantile_samples=4,
                       iqn_n_next_state_quantile_samples=4), 8, 3, True),
    "iqn_c3": (dict(use_ids=False, use_iqn=True, use_dqn=False), 256, 3, False),
    "dqn_c2": (dict(use_ids=False, use_iqn=False, use_dqn=True, use_layer_norm=False), 256, 3, True),
    "dqn_ln": (dict(use_ids=False, use_iqn=False, use_dqn=True, use_layer_norm=True), 32, 2, False),
    "dqn_target_c2": (dict(use_ids=False, use_iqn=False, use_dqn=True, use_layer_norm=False,
                           use_target_network=True), 64, 2, False),
    "full_c4": (dict(use_ids=True, use_iqn=True, use_target_network=True), 512, 2, False),
    "full_small": (dict(use_ids=True, use_iqn=True, use_target_network=True), 16, 2, False),
    "full_notarget": (dict(use_ids=True, use_iqn=True, use_target_network=False), 16, 2, False),
    "full_doubleq": (dict(use_ids=True, use_iqn=True, use_target_network=True, use_double_q_learning=True),
                     16, 2, False),
    "iqn_target": (dict(use_ids=False, use_iqn=True, use_target_network=True), 32, 2, False),
    "iqn_doubleq": (dict(use_ids=False, use_iqn=True, use_target_network=True, use_double_q_learning=True),
                    32, 2, False),
    "iqn_tau32": (dict(use_ids=False, use_iqn=True, iqn_n_current_state_quantile_samples=32,
                       iqn_n_next_state_quantile_samples=32), 16, 2, False),
    # ---- the ablation presets the reference ships (prism/config/{additive,subtractive}_ablation_base_config.py)
    # and the stages its experiment files derive from them (additive_ablation_experiment.py:31-162,
    # subtractive_ablation_experiment.py:30-52), at their own batch size (64), T = 32, width 256.
    # "base" picks the preset; the remaining keys are the stage's overrides.  "C" = observation channels
    # (MinAtar games: Breakout/Asterix 4, SpaceInvaders 6, Freeway 7, Seaquest 10).
    "abl_iqn": (dict(base="additive"), 64, 2, False),
    "abl_ln_notarget": (dict(base="additive", use_layer_norm=True, use_target_network=False), 64, 2, False),
    "abl_doubleq": (dict(base="additive", use_target_network=True, use_double_q_learning=True, C=7), 64, 2, False),
    "abl_ids": (dict(base="additive", use_ids=True, ids_n_q_head_model_layers=2, ids_n_q_heads=10,
                     ids_ensemble_variation_coef=0, ids_q_head_feature_dim=256), 64, 2, False),
    "abl_ids_var": (dict(base="additive", use_dqn=False, use_iqn=True, use_ids=True, ids_n_q_head_model_layers=2,
                         ids_n_q_heads=10, ids_q_head_feature_dim=256, ids_ensemble_variation_coef=1e-6, C=10),
                    64, 2, False),
    "abl_sub": (dict(base="subtractive", use_layer_norm=True, use_per=False, use_target_network=True,
                     target_update_period=4_000), 64, 2, False),
    # ---- the value-squish hooks of the TD target (loss_squish_fn_id; model_factory.py:16-23, iqn_model.py:141-148,
    # q_ensemble.py:77-82; the IDS selector scores unsquished estimates, action_selectors.py:128-130)
    "iqn_symlog": (dict(use_ids=False, use_iqn=True, use_dqn=False, loss_squish_fn_id="symlog"), 32, 2, False),
    "full_olf": (dict(use_ids=True, use_iqn=True, use_target_network=True, loss_squish_fn_id="obs_look_further"), 16, 2, False),
    "dqn_symlog": (dict(use_ids=False, use_iqn=False, use_dqn=True, use_layer_norm=False, loss_squish_fn_id="symlog"),
                   32, 2, False),
    # ---- the linear IQN head (iqn_quantile_model_layers = 0: no trunk, iqn_model.py:32-46), LayerNorm on and off
    "iqn_l0": (dict(use_ids=False, use_iqn=True, use_dqn=False, iqn_quantile_model_layers=0), 32, 2, False),
    "iqn_l0_noln_dq": (dict(use_ids=False, use_iqn=True, use_dqn=False, iqn_quantile_model_layers=0, use_layer_norm=False,
                            use_target_network=True, use_double_q_learning=True, iqn_n_current_state_quantile_samples=16,
                            iqn_n_next_state_quantile_samples=16, loss_squish_fn_id="symlog"), 16, 2, False),
    # ---- the optimizers beside Adam (agent_factory.py:48-58): centered RMSprop (use_adam off, use_rmsprop on), plain SGD
    "dqn_c2_rmsprop": (dict(use_ids=False, use_iqn=False, use_dqn=True, use_layer_norm=False, use_adam=False,
                            use_rmsprop=True), 256, 3, True),
    "iqn_c3_rmsprop": (dict(use_ids=False, use_iqn=True, use_dqn=False, use_adam=False, use_rmsprop=True), 256, 3, False),
    "abl_ln_notarget_rmsprop": (dict(base="additive", use_layer_norm=True, use_target_network=False, use_adam=False,
                                     use_rmsprop=True), 64, 2, False),
    "full_small_sgd": (dict(use_ids=True, use_iqn=True, use_target_network=True, use_adam=False, use_rmsprop=False),
                       16, 2, False),
    # ---- away from the presets' scalars: Huber kappa on both sides of 1, loss weights, the Theil coefficient, the clip
    # threshold below the gradient norm, Adam / RMSprop hyper-parameters (lr / eps at or below the presets' ratio).  A fifth
    # element is synth_batch's (p_term, p_short): more terminal samples and more short-walk gammas per step; a third number
    # in it is added to the seed of the batch generator -- the first offset at which the oracle's own gradient is free of
    # kink-adjacent ReLU units at the recorded inputs (tests/scalar_cases.py worst_kink <= 0.5, asserted by
    # tests/test_scalar_case_inputs.py; width 256 without LayerNorm and the ten heads meet such units at most seeds).
    # "head_scale" = (a, b): every parameter of Q head h is multiplied by a + b * h after the factory built the agent
    # (heads of equal norm leave the Theil term at ~4e-8).
    "iqn_scalars": (dict(use_ids=False, use_iqn=True, use_dqn=False, iqn_huber_loss_kappa=0.37, distributional_loss_weight=0.6,
                         max_grad_norm=0.05, **_ADAM_SCALARS), 32, 2, False, _MIXED),
    "iqn_t16_scalars": (dict(use_ids=False, use_iqn=True, use_dqn=False, use_target_network=True, use_double_q_learning=True,
                             iqn_n_current_state_quantile_samples=16, iqn_n_next_state_quantile_samples=16,
                             iqn_huber_loss_kappa=1.6, distributional_loss_weight=2.0, max_grad_norm=3.0), 16, 2, False, _MIXED),
    "iqn_l0_scalars": (dict(use_ids=False, use_iqn=True, use_dqn=False, iqn_quantile_model_layers=0, iqn_huber_loss_kappa=0.37,
                            distributional_loss_weight=0.6, **_ADAM_SCALARS), 32, 2, False, _MIXED),
    "full_scalars": (dict(use_ids=True, use_iqn=True, use_target_network=True, iqn_huber_loss_kappa=1.6,
                          distributional_loss_weight=0.3, q_loss_weight=1.7, ids_ensemble_variation_coef=0.5, max_grad_norm=0.5,
                          head_scale=(0.55, 0.1)), 16, 2, False, _MIXED + (1,)),
    "full_nodistgrad": (dict(use_ids=True, use_iqn=True, use_target_network=True, ids_allow_distributional_gradients=False,
                             iqn_huber_loss_kappa=1.6, distributional_loss_weight=0.3, q_loss_weight=1.7), 16, 2, False, _MIXED),
    "dqn_rmsprop_scalars": (dict(use_ids=False, use_iqn=False, use_dqn=True, use_layer_norm=False, q_loss_weight=0.4,
                                 use_adam=False, use_rmsprop=True, rmsprop_alpha=0.9, rmsprop_epsilon=0.02, learning_rate=5e-4,
                                 max_grad_norm=0.1), 32, 2, False, _MIXED),          # (gradient norms 0.31 - 0.45 at q weight 0.4)
    "abl_scalars": (dict(base="additive", iqn_huber_loss_kappa=0.37, distributional_loss_weight=0.6), 64, 2, False, _MIXED + (21,)),
}


def scale_heads(model, head_scale):
    """Every parameter of Q head h times a + b * h, in place."""
    a, b = head_scale
    with torch.no_grad():
        for k, p in model.named_parameters():
            if k.startswith("q_function_model.q_heads."):
                p.mul_(a + b * int(k.split(".")[2]))


def gen_update_case(name, overrides, B, steps, store_full, batch_p=None):
    from prism.config import Config, MINATAR_CONFIG, ADDITIVE_ABLATION_BASE_CONFIG, SUBTRACTIVE_ABLATION_BASE_CONFIG
    from prism.factory import agent_factory

    overrides = dict(overrides)
    base = overrides.get("base", "minatar")
    C = overrides.pop("C", 4)
    head_scale = overrides.pop("head_scale", None)
    A = 6
    preset = {"minatar": MINATAR_CONFIG, "additive": ADDITIVE_ABLATION_BASE_CONFIG,
              "subtractive": SUBTRACTIVE_ABLATION_BASE_CONFIG}[base]
    cfg = Config(**preset.__dict__)
    cfg.device, cfg.use_cuda_graph, cfg.use_e_greedy = "cpu", False, False
    for k, v in overrides.items():
        if k != "base":
            setattr(cfg, k, v)
    torch.manual_seed(cfg.seed)
    with contextlib.redirect_stdout(io.StringIO()):
        agent = agent_factory.build_agent(cfg, (10, 10, C), A)
    out = {"seed": cfg.seed, "B": B, "steps": steps, "C": C, "A": A}
    if head_scale is not None:
        scale_heads(agent.model, head_scale)
        scale_heads(agent.target_model, head_scale)
        out["head_scale"] = np.array(head_scale, np.float64)
    ov = {k: v for k, v in overrides.items() if k != "base"}
    out["base"] = base
    out["overrides_keys"] = np.array(list(ov.keys()))
    out["overrides_vals"] = np.array([repr(v) for v in ov.values()])
    names, s0, l0 = tensor_stats(agent.model.state_dict())
    out["param_names"] = np.array(names)
    out["init_sum"], out["init_l2"] = s0, l0
    out["n_params"] = sum(p.numel() for p in agent.model.parameters())
    if store_full:
        for k, v in agent.model.state_dict().items():
            out["init/" + k] = v.numpy().copy()

    rng = np.random.default_rng(1000 + sum(map(ord, name)) + (batch_p[2] if batch_p is not None and len(batch_p) > 2 else 0))
    real_rand = torch.rand
    for step in range(steps):
        b = synth_batch(rng, B, C, A) if batch_p is None else synth_batch(rng, B, C, A, *batch_p[:2])
        taus = []

        def rec(*a, **k):
            r = real_rand(*a, **k)
            taus.append(r.clone())
            return r

        torch.rand = rec
        try:
            td = agent.update(to_ref_batch(b), per_weights=torch.from_numpy(b["w"]))
        finally:
            torch.rand = real_rand
        pre = f"s{step}/"
        out[pre + "obs_bits"] = np.packbits(b["obs"].astype(np.uint8).reshape(-1))
        out[pre + "next_obs_bits"] = np.packbits(b["next_obs"].astype(np.uint8).reshape(-1))
        for k in ("reward", "nonterminal", "gamma", "action", "w"):
            out[pre + k] = b[k]
        out[pre + "n_taus"] = len(taus)
        for i, t in enumerate(taus):
            out[pre + f"tau{i}"] = t.numpy().reshape(-1)
        out[pre + "td"] = td.detach().numpy()
        if agent._static_distribution_loss is not None:
            out[pre + "dl"] = agent._static_distribution_loss.detach().numpy()
        if agent._static_q_loss is not None:
            out[pre + "ql"] = agent._static_q_loss.detach().numpy()
        out[pre + "total"] = float(agent._static_total_loss.detach())
        # grads left on the parameters are the CLIPPED ones; recover the global norm from the
        # reference's own arithmetic: clip multiplies by min(1, max/(norm+1e-6))
        gl2 = np.array([float(p.grad.double().norm()) if p.grad is not None else 0.0
                        for p in agent.model.parameters()])
        out[pre + "clipped_grad_l2"] = gl2
        n2, s, l2 = tensor_stats(agent.model.state_dict())
        out[pre + "post_sum"], out[pre + "post_l2"] = s, l2
        if agent.model.q_function_model is not None:
            out[pre + "theil"] = float(agent.model.q_function_model.theil.detach())
        if store_full and step == steps - 1:
            for k, v in agent.model.state_dict().items():
                out[pre + "post/" + k] = v.numpy().copy()
        if store_full and step == 0:
            for (k, p) in agent.model.named_parameters():
                out[pre + "clipped_grad/" + k] = p.grad.numpy().copy()
        if cfg.use_target_network and step == 0:
            agent.sync_target_model()       # exercise hard sync between steps
    # acting on the updated weights: Agent.forward's pieces (agent.py:31-41) for a handful of observations --
    # CompositeModel.forward(for_action=True), then the training-time selector's scores / choice
    n_act = 5
    act_obs = (rng.random((n_act, 10, 10, C)) < 0.1).astype(np.float32)
    torch.manual_seed(4242)
    with torch.no_grad():
        q, dist = agent.model(torch.from_numpy(act_obs), for_action=True)
    out["act/obs_bits"] = np.packbits(act_obs.astype(np.uint8).reshape(-1))
    out["act/n"] = n_act
    out["act/q"] = q.numpy()
    if cfg.use_iqn:
        T_act = cfg.iqn_quantile_samples_per_action
        torch.manual_seed(4242)
        out["act/tau"] = torch.rand([T_act * n_act, 1]).float().numpy().reshape(-1)      # the draw iqn_model.py:66-68 made
        out["act/dist"] = dist.numpy()
    sel = agent.action_selector
    with torch.no_grad():
        probs = sel.generate_action_probs(dist, q, for_log=True) if cfg.use_ids else sel.generate_action_probs(dist, q)
        out["act/action"] = sel.select_action(probs).numpy()
    out["act/probs"] = probs.numpy()
    if cfg.use_ids:
        for k, v in sel.loggables.items():
            out["act/ids/" + k] = v.numpy()
    np.savez_compressed(os.path.join(OUT, f"update_{name}.npz"), **out)
    print(f"update_{name}: P={out['n_params']} total[-1]={out[pre + 'total']:.6f} act={out['act/action'].tolist()}")


# The additional n-step chains, each `tests/golden/<name>.npz`: (n_step, gamma, rows, per stream the period of episode ends,
# per stream the period of truncations; 0 = never).  Streams of unequal episode lengths, so that the chains together hold walks
# that exhaust n_step, stop at a done, stop at a truncation and stop at a successor that is not stored yet (the open row of
# every stream at the end).  tests/helpers.py NSTEP_CHAINS lists the same names.
NSTEP_CHAINS = {
    "nstep_chain_n1": (1, 0.99, 66, (7, 5, 11), (5, 0, 4), 101),
    "nstep_chain_n2": (2, 0.5, 68, (3, 6, 0, 9), (0, 4, 5, 7), 102),
    "nstep_chain_n5": (5, 0.997, 70, (6, 13, 4, 0, 9), (11, 5, 0, 7, 0), 105),
    "nstep_chain_n15_g1": (15, 1.0, 69, (0, 9, 17), (22, 5, 0), 115),
    "nstep_chain_n15": (15, 0.99, 72, (17, 0, 6, 19), (0, 16, 11, 7), 116),
}


def _nstep_chain(n_step, gamma, rows, done_every, trunc_every, seed):
    """Timestep chains of len(done_every) interleaved env streams, as the collector links them
    (experience_collector.py:94-120), pushed through the reference's n-step + collate.  Returns (stored timesteps, arrays,
    the buffer, its stand-in ring class, keep): `keep` holds the strong references -- the streams' open successors among them,
    which the chain reaches through weak links only; whoever goes on using `stored` must hold it as long."""
    from prism.experience import Timestep, TimestepBuffer
    import weakref

    class FakeRB:
        _batch_size = 0

    rng = np.random.default_rng(seed)
    keep = []            # strong refs (links are weak)
    env_streams = len(done_every)
    O = (10, 10, 4)
    next_id = [0]

    def new_ts():
        t = Timestep(id=next_id[0])
        next_id[0] += 1
        return t

    current = []
    for e in range(env_streams):
        t = new_ts()
        t.obs = torch.from_numpy((rng.random(O) < 0.1).astype(np.float32))
        current.append(t)
    stored = []          # completed timesteps in insertion order
    steps_per_stream = [0] * env_streams
    for it in range(rows):
        e = it % env_streams
        cur = current[e]
        steps_per_stream[e] += 1
        k = steps_per_stream[e]
        done = bool(done_every[e]) and (k % done_every[e] == 0)
        trunc = (not done) and bool(trunc_every[e]) and (k % trunc_every[e] == 0)
        cur.action = int(rng.integers(0, 6))
        cur.reward = float(np.float32(rng.standard_normal()))
        cur.done, cur.truncated = bool(done), bool(trunc)
        nxt = new_ts()
        nxt.obs = torch.from_numpy((rng.random(O) < 0.1).astype(np.float32))
        if trunc:
            tr = new_ts()
            tr.obs = torch.from_numpy((rng.random(O) < 0.1).astype(np.float32))
            tr.prev = weakref.ref(cur)
            cur.next = tr
        elif not done:
            nxt.prev = weakref.ref(cur)
            cur.next = weakref.ref(nxt)
        current[e] = nxt
        stored.append(cur)
        keep.append(cur)
    keep.extend(current)

    buf = TimestepBuffer(FakeRB(), frame_stack=1, device="cpu", n_step=n_step, gamma=gamma)
    N = len(stored)
    batch = buf._timesteps_to_batch(stored, N)
    id_to_row = {t.id: i for i, t in enumerate(stored)}
    out = {"n_step": n_step, "gamma": gamma, "N": N}
    out["obs"] = np.stack([t.obs.numpy() for t in stored])
    succ = np.zeros_like(out["obs"])
    link = np.full(N, -1, np.int32)
    has_next = np.zeros(N, bool)
    for i, t in enumerate(stored):
        nx = t.next
        if nx is None:
            continue
        node = nx if isinstance(nx, Timestep) else nx()
        has_next[i] = True
        succ[i] = node.obs.numpy()
        if not isinstance(nx, Timestep) and node.reward is not None and node.id in id_to_row:
            link[i] = id_to_row[node.id]
    out["succ_obs"], out["link"], out["has_next"] = succ, link, has_next
    out["reward"] = np.array([t.reward for t in stored], np.float64)
    out["done"] = np.array([t.done for t in stored])
    out["truncated"] = np.array([t.truncated for t in stored])
    out["action"] = np.array([t.action for t in stored], np.int64)
    out["exp_n_step_return"] = np.array([t.n_step_return for t in stored], np.float64)
    out["exp_n_step_gamma"] = np.array([t.n_step_gamma for t in stored], np.float64)
    out["exp_n_step_done"] = np.array([bool(t.n_step_done) for t in stored])
    out["exp_needs_n_step"] = np.array([bool(t.needs_n_step) for t in stored])
    out["exp_batch_obs"] = batch["observation"].numpy()
    out["exp_batch_next_obs"] = batch["next"]["observation"].numpy()
    out["exp_batch_reward"] = batch["next"]["reward"].numpy()
    out["exp_batch_nonterminal"] = batch["nonterminal"].numpy()
    out["exp_batch_gamma"] = batch["gamma"].numpy()
    out["exp_batch_action"] = batch["action"].numpy()
    return stored, out, buf, FakeRB, keep


def gen_nstep_more():
    """The chains of NSTEP_CHAINS: other n-step lengths and discounts than nstep_chain.npz, which this leaves alone."""
    for name, spec in NSTEP_CHAINS.items():
        out = _nstep_chain(*spec)[1]
        np.savez_compressed(os.path.join(OUT, name + ".npz"), **out)
        print(f"{name}: n_step {spec[0]}, gamma {spec[1]}, {out['N']} timesteps; needs_n_step:",
              int(out["exp_needs_n_step"].sum()), "terminal rows:", int((~out["exp_batch_nonterminal"]).sum()))


def gen_nstep():
    """Hand-built Timestep chains pushed through the reference's n-step + collate."""
    from prism.experience import TimestepBuffer
    n_step, gamma = 3, 0.99
    # (`keep` lives to the end of this function: the open rows' successors must be alive when the reference saves the chain)
    stored, out, buf, FakeRB, keep = _nstep_chain(n_step, gamma, 67, (7, 7, 7), (5, 5, 5), 7)
    N = out["N"]
    np.savez_compressed(os.path.join(OUT, "nstep_chain.npz"), **out)
    print("nstep_chain:", N, "timesteps; needs_n_step:", int(out["exp_needs_n_step"].sum()),
          "terminal rows:", int((~out["exp_batch_nonterminal"]).sum()))

    # ---- the same chain through the reference's buffer checkpoint: TimestepBuffer.save -> timesteps.pkl, then its
    # own load and collate again (timestep_buffer.py:259-318).  The torchrl sampler / writer dumps are absent here:
    # stand-ins that write nothing.
    class Dumper:
        def dumps(self, path):
            pass

        def loads(self, path):
            pass

    rb = FakeRB()
    rb._storage = [[t] for t in stored]
    rb._sampler, rb._writer = Dumper(), Dumper()
    buf.buffer = rb
    ck = os.path.join(OUT, "ref_buffer")
    with contextlib.redirect_stdout(io.StringIO()):
        buf.save(ck)
        rb2 = FakeRB()
        rb2._storage = [None] * N
        rb2._sampler, rb2._writer = Dumper(), Dumper()
        buf2 = TimestepBuffer(rb2, frame_stack=1, device="cpu", n_step=n_step, gamma=gamma)
        buf2.load(ck)
    kept = [s_[0] for s_ in rb2._storage if s_ is not None]
    batch2 = buf2._timesteps_to_batch(kept, len(kept))
    np.savez_compressed(os.path.join(OUT, "ref_buffer_expected.npz"), n=len(kept), ids=np.array([t.id for t in kept]),
                        obs=batch2["observation"].numpy(), next_obs=batch2["next"]["observation"].numpy(),
                        reward=batch2["next"]["reward"].numpy(), nonterminal=batch2["nonterminal"].numpy(),
                        gamma=batch2["gamma"].numpy(), action=batch2["action"].numpy())
    print("ref_buffer: saved", N, "timesteps, the reference's own load keeps", len(kept))
    del keep


def gen_checkpoint():
    """A checkpoint directory written by the reference's Agent.save (agent.py:179-203) after two updates of a small
    DQN agent with an epsilon-greedy selector, plus a state dict holding an IDS selector: files as the reference
    wrote them (tensors + pickled selector objects)."""
    import pickle
    import shutil
    from prism.config import Config, MINATAR_CONFIG
    from prism.factory import agent_factory
    from prism.agents.action_selectors import IDSActionSelector
    cfg = Config(**MINATAR_CONFIG.__dict__)
    cfg.device, cfg.use_cuda_graph = "cpu", False
    for k, v in dict(use_ids=False, use_iqn=False, use_dqn=True, use_layer_norm=False, use_e_greedy=True,
                     use_target_network=True).items():
        setattr(cfg, k, v)
    torch.manual_seed(cfg.seed)
    with contextlib.redirect_stdout(io.StringIO()):
        agent = agent_factory.build_agent(cfg, (10, 10, 4), 6)
    rng = np.random.default_rng(99)
    for _ in range(2):
        b = synth_batch(rng, 32)
        agent.update(to_ref_batch(b), per_weights=torch.from_numpy(b["w"]))
    agent.action_selector.epsilon.update(1234)
    ck = os.path.join(OUT, "ref_checkpoint")
    shutil.rmtree(ck, ignore_errors=True)
    agent.save(ck)
    names, s, l2 = tensor_stats(agent.model.state_dict())
    opt = agent.optimizer.state_dict()
    np.savez_compressed(os.path.join(OUT, "ref_checkpoint_expected.npz"), param_names=np.array(names), sum=s, l2=l2,
                        n_updates=agent.n_updates, max_grad_norm=agent.max_grad_norm, epsilon_step=1234,
                        adam_step=float(opt["state"][0]["step"]),
                        exp_avg_l2=np.array([float(opt["state"][i]["exp_avg"].double().norm()) for i in range(len(names))]))
    ids = IDSActionSelector(lmbda=0.1, random_sample=False, epsilon=1e-10, ids_rho_lower_bound=0.25, beta=0.8)
    with open(os.path.join(ck, "state_ids.pkl"), "wb") as f:
        pickle.dump({"action_selector": ids, "n_updates": 7}, f)
    print("ref_checkpoint:", sorted(os.listdir(os.path.join(ck, "agent"))))


def gen_checkpoint_rmsprop():
    """The same for the centered-RMSprop optimizer (agent_factory.py:48-54): the DQN model of case dqn_c2 after two
    updates, with per-tensor sums of the parameters and of the optimizer state torch wrote."""
    import shutil
    from prism.config import Config, MINATAR_CONFIG
    from prism.factory import agent_factory
    cfg = Config(**MINATAR_CONFIG.__dict__)
    cfg.device, cfg.use_cuda_graph, cfg.use_e_greedy = "cpu", False, False
    for k, v in CASES["dqn_c2_rmsprop"][0].items():
        setattr(cfg, k, v)
    torch.manual_seed(cfg.seed)
    with contextlib.redirect_stdout(io.StringIO()):
        agent = agent_factory.build_agent(cfg, (10, 10, 4), 6)
    rng = np.random.default_rng(199)
    for _ in range(2):
        b = synth_batch(rng, 32)
        agent.update(to_ref_batch(b), per_weights=torch.from_numpy(b["w"]))
    ck = os.path.join(OUT, "ref_checkpoint_rmsprop")
    shutil.rmtree(ck, ignore_errors=True)
    agent.save(ck)
    names, s, l2 = tensor_stats(agent.model.state_dict())
    opt = agent.optimizer.state_dict()
    n = len(names)
    np.savez_compressed(os.path.join(OUT, "ref_checkpoint_rmsprop_expected.npz"), param_names=np.array(names), sum=s, l2=l2,
                        n_updates=agent.n_updates, max_grad_norm=agent.max_grad_norm,
                        step=float(opt["state"][0]["step"]),
                        square_avg_sum=np.array([float(opt["state"][i]["square_avg"].double().sum()) for i in range(n)]),
                        grad_avg_sum=np.array([float(opt["state"][i]["grad_avg"].double().sum()) for i in range(n)]),
                        group_keys=np.array(sorted(k for k in opt["param_groups"][0] if k != "params")),
                        lr=opt["param_groups"][0]["lr"], alpha=opt["param_groups"][0]["alpha"],
                        eps=opt["param_groups"][0]["eps"])
    print("ref_checkpoint_rmsprop:", sorted(os.listdir(os.path.join(ck, "agent"))))


COLLECTOR_STREAMS, COLLECTOR_STEPS, COLLECTOR_EMA = 3, 60, 0.9


def collector_script(seed=41):
    """(reward float32 [streams][steps], done, truncated): fp32-representable rewards -- 0, +-1, their fp32 neighbours on
    both sides, fractions and values large enough that a float32 sum would differ from the float64 one -- and an episode
    pattern with a done on a stream's very first step, a truncation, done and truncated together, and one-step episodes."""
    rng = np.random.default_rng(seed)
    one = np.float32(1.0)
    pool = np.array([0.0, 1.0, -1.0, np.nextafter(one, np.float32(0)), np.nextafter(one, np.float32(2)),
                     np.nextafter(-one, np.float32(0)), np.nextafter(-one, np.float32(-2)), 0.5, -0.25, 3.0, -7.5, 1e6,
                     -123456.0, 16777216.0, 1e-3, -0.1], np.float32)
    S, T = COLLECTOR_STREAMS, COLLECTOR_STEPS
    reward = pool[rng.integers(0, len(pool), (S, T))]
    done = rng.random((S, T)) < 0.08
    trunc = rng.random((S, T)) < 0.05
    done[0, 0], trunc[0, 0] = True, False                      # done on a stream's first step
    done[1, 5], trunc[1, 5] = False, True                      # a truncation
    done[1, 11], trunc[1, 11] = True, True                     # both at once ...
    done[1, 12], trunc[1, 12] = True, False                    # ... and a one-step episode right behind it
    done[2, 30], trunc[2, 30] = True, False
    done[2, 31], trunc[2, 31] = False, True                    # a one-step episode ended by a truncation
    return reward, done, trunc


def gen_collector_bookkeeping():
    """What the reference's collector does to a timestep besides storing it: the live
    CollectorProcessInterface.receive_env_step (reward clip, episodic_reward) behind a stub memory interface -- no
    processes -- and ExperienceCollector.collect_timesteps around it for the training-reward EMA.  Three streams in
    lockstep, so their timesteps reach the buffer interleaved; recorded per timestep, in the order they reach it."""
    from multiprocessing_experience_collection import CollectorProcessInterface, EnvProcessMemoryInterface as E
    from multiprocessing_experience_collection import ExperienceCollector

    class StubMemory:
        def __init__(self, reward, done, trunc):
            self.reward, self.done, self.trunc, self.k, self.status = reward, done, trunc, 0, E.PROC_STATUS_WROTE_RESET_FLAG

        def set_flag(self, idx, flag):
            pass

        def get_flag(self, idx):
            return self.status if idx == E.PROC_STATUS_IDX else E.PROC_STATUS_NULL_FLAG

        def read_reset_obs(self):
            self.status = E.PROC_STATUS_WAITING_FOR_ACTION_FLAG
            return np.zeros((1, 2), np.float32), 1

        def read_step_data(self):
            k = self.k
            self.k += 1
            data = self.reward[k:k + 1]                        # a float32 slice, as shared_memory_interface.py:138 reads it
            o = np.full((1, 2), k, np.float32)
            return o, [float(r) for r in data], bool(self.done[k]), bool(self.trunc[k]), o + 1, 1, 1

        def write_action(self, action, idx):
            pass

        def send_actions(self):
            pass

    class Agent:
        def forward(self, obs):
            return torch.zeros(obs.shape[0], dtype=torch.long)

    reward, done, trunc = collector_script()
    S, T = reward.shape
    out = dict(ema=COLLECTOR_EMA, n_streams=S, n_steps=T, raw_reward=reward, script_done=done, script_truncated=trunc)
    for tag, clip in (("none", None), ("clamp", "dopamine_clamp")):
        col = ExperienceCollector.__new__(ExperienceCollector)         # __init__ without its processes
        col._device, col._timestep_id, col._inference_buffer_size = "cpu", 0, 1
        col._training_reward_ema, col._training_reward = COLLECTOR_EMA, None
        col._waiting_observations, col._waiting_timesteps, col._waiting_pids, col._action_pids = [], [], [], []
        col._buffer_idx, col._random_agent = 0, None
        col._running_processes = {e: CollectorProcessInterface(None, StubMemory(reward[e], done[e], trunc[e]), 1,
                                                               reward_clipping_type=clip) for e in range(S)}
        rows = []

        class Buffer:
            def extend(self, t):                                        # called right behind the EMA lines
                rows.append((t, col._training_reward))

        col.signal_processes_start_collecting(Agent())
        assert col.collect_timesteps(S * T, Agent(), Buffer()) == S * T
        ts = [r[0] for r in rows]
        # the stream of a row: lockstep, one timestep per stream and round, in stream order
        out[tag + "_stream"] = np.arange(S * T, dtype=np.int32) % S
        stored = np.array([t.reward for t in ts], np.float64)
        assert (stored.astype(np.float32).astype(np.float64) == stored).all()
        out[tag + "_stored_reward"] = stored.astype(np.float32)
        out[tag + "_episodic_reward"] = np.array([t.episodic_reward for t in ts], np.float64)
        out[tag + "_done"] = np.array([t.done for t in ts], np.bool_)
        out[tag + "_truncated"] = np.array([t.truncated for t in ts], np.bool_)
        out[tag + "_training_valid"] = np.array([r[1] is not None for r in rows], np.bool_)
        out[tag + "_training_reward"] = np.array([0.0 if r[1] is None else r[1] for r in rows], np.float64)
        for e in range(S):                                              # the rows are the script, interleaved
            assert (out[tag + "_done"][e::S] == done[e]).all() and (out[tag + "_truncated"][e::S] == trunc[e]).all()
    np.savez_compressed(os.path.join(OUT, "collector_bookkeeping.npz"), **out)
    ends = out["none_done"] | out["none_truncated"]
    print("collector_bookkeeping:", S * T, "timesteps,", int(ends.sum()), "episode ends, clamped rewards:",
          int((out["clamp_stored_reward"] != out["none_stored_reward"]).sum()))


def evaluator_scripts(seed=53):
    """name -> (reward float64 [steps] of float32-exact values, kind uint8 [steps]: 0 goes on | 1 done | 2 truncated |
    3 both, horizon).  Every script is longer than the evaluator can consume."""
    rng = np.random.default_rng(seed)
    pool = np.array([0.0, 1.0, -1.0, 0.5, -0.25, 3.0, -7.5, 0.1, -0.1, 1e-3, 1e6, -123456.0, 0.7, -2.59], np.float32)

    def script(lengths, kinds=None, steps=None, values=pool):
        steps = sum(lengths) if steps is None else steps
        kind = np.zeros(steps, np.uint8)
        ends = np.cumsum(lengths) - 1
        kind[ends[ends < steps]] = 1 if kinds is None else np.asarray(kinds, np.uint8)[:int((ends < steps).sum())]
        return values[rng.integers(0, len(values), steps)].astype(np.float64), kind

    runs = {}
    runs["horizon_zero"] = script([7, 3, 5]) + (0,)                        # at least one episode is still collected
    runs["on_an_end"] = script([5, 4, 6, 5]) + (9,)                        # the horizon falls on the second episode's end
    runs["before_an_end"] = script([5, 4, 6, 5]) + (8,)
    runs["after_an_end"] = script([5, 4, 6, 5]) + (10,)
    runs["long_first_episode"] = script([50, 6, 6]) + (20,)                # goes on until the first episode ends
    runs["one_step_episodes"] = script([1] * 16) + (12,)
    runs["done_and_truncated"] = script([3, 1, 4, 2, 6, 1, 5, 3, 7, 4, 6, 8],
                                        [1, 2, 3, 2, 1, 1, 2, 3, 1, 2, 1, 1]) + (40,)
    small = np.array([-0.1, 0.1, 0.7, -2.59, 1e-3, -0.25, 0.5, -7.5], np.float32)
    lengths = [int(x) for x in rng.integers(1, 30, 40)]
    runs["negative_and_fractional"] = script(lengths, [int(x) for x in rng.integers(1, 4, 40)], values=small) + (250,)
    return runs


def gen_evaluator():
    """The live SyncAgentEvaluator, loaded file-wise (the package import pulls in wandb and the environment factories),
    with a stub agent over scripted single-environment runs.  The reward arrays are float64 whose values are
    float32-exact: the evaluator's `current_ep_rew += rew[0]` then sums in float64 (with float32 arrays NumPy 2 keeps
    the sum in float32)."""
    import importlib.util
    names = ("prism", "prism.util", "prism.util.observation_stacker")
    saved = {n: sys.modules.get(n) for n in names}

    def load(name, path):
        spec = importlib.util.spec_from_file_location(name, os.path.join(REF, path))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod
    try:
        for n in names[:2]:
            sys.modules[n] = types.ModuleType(n)
            sys.modules[n].__path__ = []
        sys.modules[names[2]] = load(names[2], "prism/util/observation_stacker.py")
        SyncAgentEvaluator = load("_ref_sync_agent_evaluator", "prism/evals/sync_agent_evaluator.py").SyncAgentEvaluator
    finally:
        for n, m in saved.items():
            if m is None:
                sys.modules.pop(n, None)
            else:
                sys.modules[n] = m

    class Env:
        def __init__(self, reward, kind):
            self.reward, self.kind, self.k, self.resets = reward, kind, 0, 0

        def reset(self):
            self.resets += 1
            return np.zeros((1, 2), np.float32), {}

        def step(self, action):
            k = self.k
            self.k += 1
            return (np.full((1, 2), k, np.float32), self.reward[k:k + 1], bool(self.kind[k] & 1), bool(self.kind[k] & 2), {})

    class Agent:
        model = types.SimpleNamespace(device="cpu")

        def forward(self, obs):
            return torch.zeros(obs.shape[0], dtype=torch.long)

        def eval(self):
            pass

        def train(self):
            pass

    out, runs = {}, evaluator_scripts()
    for name, (reward, kind, horizon) in runs.items():
        assert reward.dtype == np.float64 and (reward.astype(np.float32).astype(np.float64) == reward).all()
        env = Env(reward, kind)
        ep = SyncAgentEvaluator(Agent(), env, 0, horizon).evaluate_agent()
        assert env.resets == 1 + len(ep) and len(ep) >= 1 and env.k <= len(reward)
        out[name + "_reward"], out[name + "_kind"], out[name + "_horizon"] = reward, kind, np.int64(horizon)
        out[name + "_ep_rews_bits"] = np.array([float(r) for r in ep], np.float64).view(np.uint64)
        out[name + "_timesteps"] = np.int64(env.k)
        print("evaluator:", name, "horizon", horizon, "->", len(ep), "episodes in", env.k, "timesteps")
    out["names"] = np.array(list(runs))
    np.savez_compressed(os.path.join(OUT, "evaluator_runs.npz"), **out)


def main():
    os.makedirs(OUT, exist_ok=True)
    _import_reference()
    which = sys.argv[1:] or (list(CASES) + ["nstep", "nstep_more", "config", "checkpoint", "checkpoint_rmsprop",
                                   "collector", "evaluator"])
    for name in which:
        if name == "nstep":
            gen_nstep()
        elif name == "nstep_more":
            gen_nstep_more()
        elif name == "checkpoint":
            gen_checkpoint()
        elif name == "checkpoint_rmsprop":
            gen_checkpoint_rmsprop()
        elif name == "config":
            gen_config_snapshot()
        elif name == "collector":
            gen_collector_bookkeeping()
        elif name == "evaluator":
            gen_evaluator()
        else:
            gen_update_case(name, *CASES[name])




def gen_config_snapshot():
    """Field names / order / preset values of the reference's Config, as data."""
    import dataclasses
    import json
    from prism.config import (Config, DEFAULT_CONFIG, MINATAR_CONFIG, ADDITIVE_ABLATION_BASE_CONFIG,
                              SUBTRACTIVE_ABLATION_BASE_CONFIG)
    snap = {"fields": [f.name for f in dataclasses.fields(Config)],
            "DEFAULT_CONFIG": DEFAULT_CONFIG.__dict__, "MINATAR_CONFIG": MINATAR_CONFIG.__dict__,
            "ADDITIVE_ABLATION_BASE_CONFIG": ADDITIVE_ABLATION_BASE_CONFIG.__dict__,
            "SUBTRACTIVE_ABLATION_BASE_CONFIG": SUBTRACTIVE_ABLATION_BASE_CONFIG.__dict__}
    # every configuration the two experiment files generate, as {group name: fields that differ from the base}
    # (seed 0 of each group; seeds only change `seed` / names / checkpoint_dir)
    from prism.experiments.experiment_files.additive_ablation_experiment import AdditiveAblationExperiment
    from prism.experiments.experiment_files.subtractive_ablation_experiment import SubtractiveAblationExperiment
    skip = {"seed", "wandb_project_name", "wandb_group_name", "wandb_run_name", "checkpoint_dir"}
    for key, exp_cls, base in (("ADDITIVE_STAGES", AdditiveAblationExperiment, ADDITIVE_ABLATION_BASE_CONFIG),
                               ("SUBTRACTIVE_STAGES", SubtractiveAblationExperiment, SUBTRACTIVE_ABLATION_BASE_CONFIG)):
        stages = {}
        for cfg in exp_cls(num_seeds=1).configs:
            diff = {k: v for k, v in cfg.__dict__.items() if k not in skip and base.__dict__.get(k) != v}
            stages[cfg.wandb_group_name] = diff
        snap[key] = stages
    with open(os.path.join(OUT, "config_presets.json"), "w") as f:
        json.dump(snap, f, indent=1, sort_keys=True)
    print("config_presets:", len(snap["fields"]), "fields")


if __name__ == "__main__":
    main()
