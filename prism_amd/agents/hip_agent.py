"""``HipAgent`` — duck-types the reference ``Agent`` (``/root/reference/prism/agents/agent.py``)
with the TD update running in the hand-written gfx950 kernels behind ``prism_learner_fwd_bwd`` /
``prism_learner_clip_adam`` (``prism_learner_clip_step`` for RMSprop / SGD).

Memory model: ONE flat fp32 parameter buffer per network in ``model.parameters()`` order
(SURVEY.md Appendix B); every ``nn.Parameter`` of the container modules is a view into it, so
``state_dict()`` / checkpoints interchange with the reference while the kernels and the RCCL
all-reduce see a single contiguous buffer.  Optimizer state and the gradient are flat buffers too.

Data-parallel: ``torch.distributed`` all-reduce (RCCL over xGMI) of the flat gradient sits
between the two native calls; clip + Adam then run redundantly on every rank so replicas stay
bit-identical.
"""
import contextlib
import ctypes
import gc
import os

import numpy as np
import torch

from prism_amd import _native as N
from prism_amd import dist as pdist
from prism_amd.util import ref_pickle


@contextlib.contextmanager
def graph_capture(g, **kwargs):
    """``torch.cuda.graph(g)`` with Python's cyclic garbage collector held off until the capture has ended.  A collection
    that an allocation triggers inside the capture would run the destructors of unreachable objects there -- a dropped
    agent is such garbage (its model's load hook refers back to it) and takes hipGraphs, events and pinned buffers with
    it -- and a HIP call from one of those in the middle of a capture aborts the process."""
    enabled = gc.isenabled()
    gc.disable()
    try:
        with torch.cuda.graph(g, **kwargs):
            yield
    finally:
        if enabled:
            gc.enable()


class HipOptimizer:
    """Flat optimizer state behind a ``torch.optim`` ``state_dict`` (the update itself is the fused kernel): ``exp_avg``
    style names per kind in the subclasses, ``buffers()`` = the flat fp32 tensors that hold them, ``native_buffers()`` = the
    two ``prism_learner_desc.adam_m`` / ``adam_v`` point at, ``step_t`` = the device step counter every kind advances.  One
    subclass per optimizer agent_factory.py:40-58 builds."""
    kind = None                   # PRISM_OPT_* (include/prism_hip.h)
    state_names = ()              # torch's per-parameter state keys held in buffers()[0], buffers()[1]

    def __init__(self, named_params, flat_params):
        self.names = [n for n, _ in named_params]
        self.shapes = [tuple(p.shape) for _, p in named_params]
        self.numels = [p.numel() for _, p in named_params]
        self.flat_params = flat_params
        self.step_t = torch.zeros(1, dtype=torch.int64, device=flat_params.device)

    def zero_grad(self, set_to_none=True):
        pass

    def buffers(self):
        raise NotImplementedError

    def native_buffers(self):
        """What ``prism_learner_desc.adam_m`` / ``adam_v`` point at (include/prism_hip.h: first and second moment; both
        must be valid pointers for every kind)."""
        return self.buffers()

    def native_hyper(self):
        """``prism_opt_hyper`` of the current param group (None: Adam, whose hyper-parameters travel in
        ``prism_learner_desc.hyper``)."""
        return None

    def hyper_key(self):
        """Everything of the param group a captured launch bakes beyond ``prism_learner_desc.hyper`` (the step graph is
        keyed by it; None: Adam)."""
        return None

    def state_dict(self):
        state, off = {}, 0
        step = float(self.step_t.item())
        bufs = self.buffers()
        for i, (n, shp) in enumerate(zip(self.numels, self.shapes)):
            if step > 0 and self.state_names:
                st = {"step": torch.tensor(step)}
                for name, buf in zip(self.state_names, bufs):
                    st[name] = buf[off:off + n].view(shp).clone()
                state[i] = st
            off += n
        return {"state": state, "param_groups": [dict(g) for g in self.param_groups]}

    def load_state_dict(self, sd, keys=()):
        off, step = 0, 0
        bufs = self.buffers()
        for i, (n, shp) in enumerate(zip(self.numels, self.shapes)):
            st = sd["state"].get(i)
            if st is not None and self.state_names:
                for name, buf in zip(self.state_names, bufs):
                    buf[off:off + n].copy_(st[name].reshape(-1))
                step = int(float(st["step"]))
            off += n
        if self.state_names:          # (SGD's files carry no step count: the counter stays where it is)
            self.step_t.fill_(step)
        if sd.get("param_groups"):
            g = sd["param_groups"][0]
            for k in keys:
                if k in g:
                    self.param_groups[0][k] = g[k]


class HipAdam(HipOptimizer):
    """``torch.optim.Adam``, options of agent_factory.py:44-47."""
    kind = N.OPT_ADAM
    state_names = ("exp_avg", "exp_avg_sq")

    def __init__(self, named_params, flat_params, lr, betas, eps):
        super().__init__(named_params, flat_params)
        self.exp_avg = torch.zeros_like(flat_params)
        self.exp_avg_sq = torch.zeros_like(flat_params)
        self.param_groups = [dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=0, amsgrad=False,
                                  maximize=False, foreach=None, capturable=False, differentiable=False,
                                  fused=None, params=list(range(len(self.names))))]

    def buffers(self):
        return self.exp_avg, self.exp_avg_sq

    def load_state_dict(self, sd):
        super().load_state_dict(sd, keys=("lr", "betas", "eps"))


def _torch_param_group(opt_cls, n_params, **kw):
    """The param group the installed ``torch.optim`` class writes for these options (its own key set and defaults), with
    the parameters numbered as its ``state_dict()`` numbers them."""
    g = dict(opt_cls([torch.zeros(1)], **kw).param_groups[0])
    g["params"] = list(range(n_params))
    return g


class HipRMSprop(HipOptimizer):
    """``torch.optim.RMSprop(lr, alpha, eps, centered=True)`` (agent_factory.py:48-54): per-parameter ``step``,
    ``square_avg``, ``grad_avg`` in torch's own layout."""
    kind = N.OPT_RMSPROP
    state_names = ("square_avg", "grad_avg")

    def __init__(self, named_params, flat_params, lr, alpha, eps):
        super().__init__(named_params, flat_params)
        self.grad_avg = torch.zeros_like(flat_params)
        self.square_avg = torch.zeros_like(flat_params)
        self.param_groups = [_torch_param_group(torch.optim.RMSprop, len(self.names), lr=lr, alpha=alpha, eps=eps,
                                                centered=True)]

    def buffers(self):
        return self.square_avg, self.grad_avg

    def native_buffers(self):
        return self.grad_avg, self.square_avg

    def native_hyper(self):
        g = self.param_groups[0]
        return N.OptHyper(self.kind, float(g["lr"]), float(g["alpha"]), float(g["eps"]))

    def hyper_key(self):
        g = self.param_groups[0]
        return ("rmsprop", g["lr"], g["alpha"], g["eps"])

    def load_state_dict(self, sd):
        g = (sd.get("param_groups") or [{}])[0]
        if not g.get("centered", True) or g.get("momentum", 0) or g.get("weight_decay", 0):
            raise ValueError("prism_amd: RMSprop state with centered=False, momentum or weight decay "
                             "(the kernel implements the form agent_factory.py:48-54 builds)")
        super().load_state_dict(sd, keys=("lr", "alpha", "eps"))


class HipSGD(HipOptimizer):
    """``torch.optim.SGD(lr)`` (agent_factory.py:56-58): no per-parameter state.  The two state pointers of the descriptor
    must still be valid: one 16-byte block serves both."""
    kind = N.OPT_SGD

    def __init__(self, named_params, flat_params, lr):
        super().__init__(named_params, flat_params)
        self._unused = torch.zeros(4, dtype=torch.float32, device=flat_params.device)
        self.param_groups = [_torch_param_group(torch.optim.SGD, len(self.names), lr=lr)]

    def buffers(self):
        return self._unused, self._unused

    def native_hyper(self):
        return N.OptHyper(self.kind, float(self.param_groups[0]["lr"]), 0.0, 0.0)

    def hyper_key(self):
        return ("sgd", self.param_groups[0]["lr"])

    def load_state_dict(self, sd):
        g = (sd.get("param_groups") or [{}])[0]
        if g.get("momentum", 0) or g.get("weight_decay", 0) or g.get("nesterov", False):
            raise ValueError("prism_amd: SGD state with momentum / weight decay (the kernel implements plain SGD)")
        super().load_state_dict(sd, keys=("lr",))


def build_optimizer(config, named_params, flat_params):
    """The reference's three-way choice with its precedence (agent_factory.py:40-58): ``use_adam`` wins, then
    ``use_rmsprop``, else SGD."""
    if config.use_adam:
        return HipAdam(named_params, flat_params, config.learning_rate, (config.adam_beta1, config.adam_beta2),
                       config.adam_epsilon)
    if config.use_rmsprop:
        return HipRMSprop(named_params, flat_params, config.learning_rate, config.rmsprop_alpha, config.rmsprop_epsilon)
    return HipSGD(named_params, flat_params, config.learning_rate)


def _flatten_into(model, device):
    """Move every parameter into one contiguous fp32 buffer (parameters() order) and re-point the
    parameters at views of it."""
    params = list(model.parameters())
    flat = torch.empty(sum(p.numel() for p in params), dtype=torch.float32, device=device)
    off = 0
    for p in params:
        n = p.numel()
        flat[off:off + n].copy_(p.data.reshape(-1))
        p.data = flat[off:off + n].view(p.shape)
        off += n
    return flat


def _offsets(model):
    """state_dict key -> flat offset, mapped onto the C ABI's prism_param_offsets."""
    off, table = 0, {}
    for name, p in model.named_parameters():
        table[name] = off
        off += p.numel()
    o = N.ParamOffsets()
    for f, _ in N.ParamOffsets._fields_:
        setattr(o, f, -1)
    o.n_params = off
    g = table.get
    o.conv_w, o.conv_b = g("embedding_model.model.0.weight", -1), g("embedding_model.model.0.bias", -1)
    d = "distribution_model."
    o.phi_w, o.phi_b = g(d + "phi.0.weight", -1), g(d + "phi.0.bias", -1)
    # LayerNorm on: trunk [LN, Linear, ReLU], head [LN, Linear].  Decided by the head: a model without a trunk
    # (iqn_quantile_model_layers = 0, iqn_model.py:32-46) has no model.model.* at all and keeps every trunk field at -1
    if d + "embedding_to_quantile_layer.1.weight" in table:
        o.iqn_ln1_g, o.iqn_ln1_b = g(d + "model.model.0.weight", -1), g(d + "model.model.0.bias", -1)
        o.iqn_w1, o.iqn_b1 = g(d + "model.model.1.weight", -1), g(d + "model.model.1.bias", -1)
        o.iqn_ln2_g = g(d + "embedding_to_quantile_layer.0.weight", -1)
        o.iqn_ln2_b = g(d + "embedding_to_quantile_layer.0.bias", -1)
        o.iqn_w2 = g(d + "embedding_to_quantile_layer.1.weight", -1)
        o.iqn_b2 = g(d + "embedding_to_quantile_layer.1.bias", -1)
    else:                                            # use_layer_norm=False: [Linear, ReLU] / Linear (iqn_model.py:42-46)
        o.iqn_w1, o.iqn_b1 = g(d + "model.model.0.weight", -1), g(d + "model.model.0.bias", -1)
        o.iqn_w2 = g(d + "embedding_to_quantile_layer.weight", -1)
        o.iqn_b2 = g(d + "embedding_to_quantile_layer.bias", -1)
    heads = sorted({int(k.split(".")[2]) for k in table if k.startswith("q_function_model.q_heads.")})
    if heads:
        pre = "q_function_model.q_heads.0."
        names = [k[len(pre):] for k in table if k.startswith(pre)]
        o.head_base = min(table[pre + n] for n in names)
        if len(heads) > 1:
            o.head_stride = table["q_function_model.q_heads.1." + names[0]] - table[pre + names[0]]
        else:
            o.head_stride = 0
        rel = {n: table[pre + n] - o.head_base for n in names}
        # FFNN-style head: model.{0:LN,1:Linear,3:LN,4:Linear} | model.{0:Linear} | model.{0:LN,1:Linear}
        order = sorted(rel, key=lambda n: rel[n])
        lin = [n[:-len(".weight")] for n in order if n.endswith(".weight") and (n[:-len(".weight")] + ".bias") in rel
               and len(dict(model.named_parameters())[pre + n].shape) == 2]
        lns = [n[:-len(".weight")] for n in order if n.endswith(".weight") and n[:-len(".weight")] not in lin]
        if len(lin) >= 1:
            o.h_w1, o.h_b1 = rel[lin[0] + ".weight"], rel[lin[0] + ".bias"]
        if len(lin) >= 2:
            o.h_w2, o.h_b2 = rel[lin[1] + ".weight"], rel[lin[1] + ".bias"]
        if len(lns) >= 1:
            o.h_ln1_g, o.h_ln1_b = rel[lns[0] + ".weight"], rel[lns[0] + ".bias"]
        if len(lns) >= 2:
            o.h_ln2_g, o.h_ln2_b = rel[lns[1] + ".weight"], rel[lns[1] + ".bias"]
    return o


def model_dims(config, in_channels, n_actions):
    d = N.ModelDims()
    d.in_channels, d.n_actions, d.embed_dim = int(in_channels), int(n_actions), 1024
    d.use_iqn = int(bool(config.use_iqn))
    d.n_basis, d.iqn_layers = config.iqn_n_basis_elements, config.iqn_quantile_model_layers
    d.iqn_width = config.iqn_quantile_model_feature_dim
    d.n_tau, d.n_tau_next = config.iqn_n_current_state_quantile_samples, config.iqn_n_next_state_quantile_samples
    d.use_layer_norm = int(bool(config.use_layer_norm))
    if config.use_ids:
        d.n_heads, d.head_layers, d.head_width = (config.ids_n_q_heads, config.ids_n_q_head_model_layers,
                                                  config.ids_q_head_feature_dim)
        d.theil_coef = config.ids_ensemble_variation_coef
    elif config.use_dqn:
        d.n_heads, d.head_layers, d.head_width = 1, config.dqn_n_model_layers, config.dqn_n_model_feature_dim
        d.theil_coef = 0.0
    d.has_target = int(bool(config.use_target_network))
    d.double_q = int(bool(config.use_double_q_learning))
    d.propagate_grad = int((config.ids_allow_distributional_gradients and config.use_ids) or not config.use_ids)
    d.huber_k, d.dist_loss_weight = config.iqn_huber_loss_kappa, config.distributional_loss_weight
    d.q_loss_weight = config.q_loss_weight
    from prism_amd.agents.squish_functions import SQUISH_IDS
    d.squish_fn = SQUISH_IDS.get(str(config.loss_squish_fn_id), 0)       # (unknown ids parse to no squish, model_factory.py:16-23)
    return d


class _Actions(torch.Tensor):
    """What ``HipAgent.forward`` returns when it ran from its hipGraph: a device tensor like the reference's
    (agent.py:41), whose ``.cpu()`` -- what every collector / evaluator calls next (experience_collector.py:127) -- hands
    out the copy the graph's own device-to-host node already made into pinned memory: one event wait instead of a second
    copy and a device synchronisation."""

    @staticmethod
    def wrap(dev, host, event):
        t = dev.as_subclass(_Actions)
        t._host, t._event = host, event
        return t

    def cpu(self, *a, **k):
        host = getattr(self, "_host", None)
        if host is None:
            return torch.Tensor.cpu(self.as_subclass(torch.Tensor), *a, **k)
        self._event.synchronize()
        return host.clone()

    def numpy(self, *a, **k):
        return self.cpu().numpy()

    def tolist(self):
        return self.cpu().tolist()

    def item(self):
        return self.cpu().item()


class _DrawCount:
    """What ``HipAgent.acting_stream`` hands back: ``count``, the acting draw count its block reached."""

    def __init__(self, count):
        self.count = count


class HipAgent:
    CURSOR_FORM = "either slot"               # _fused_key's `form` for a capture whose graphs bake one cursor slot each

    def __init__(self, model, action_selector, eval_action_selector, target_model, config, in_channels,
                 n_actions, process_group=None):
        if not str(config.device).startswith("cuda"):
            raise N.NativeLibraryError("HipAgent needs a GPU device; prism_amd has no CPU fallback")
        N.lib()
        self.device = torch.device(config.device)
        self.config = config
        self.model, self.target_model = model, target_model
        self.action_selector, self.eval_action_selector = action_selector, eval_action_selector
        self.max_grad_norm = config.max_grad_norm
        self.use_cuda_graph = False
        self.n_updates = 0
        self._is_eval = False
        self._static_batch = None
        self._static_distribution_loss = None
        self._static_q_loss = None
        self._static_total_loss = None

        self.flat = _flatten_into(model, self.device)
        self.flat_target = _flatten_into(target_model, self.device) if target_model is not None else None
        self.grads = torch.zeros_like(self.flat)
        self.optimizer = build_optimizer(config, list(model.named_parameters()), self.flat)
        # Adam runs through prism_learner_clip_adam / prism_step_back; the other kinds through prism_learner_clip_step /
        # prism_step_back_opt (config.optimizer_entry_points = True sends Adam through those too: same kernels, same bits)
        self._opt_calls = self.optimizer.kind != N.OPT_ADAM or bool(getattr(config, "optimizer_entry_points", False))
        # what a captured launch bakes of the hyper-parameters beyond prism_learner_desc.hyper.  None IS "the optimizer is
        # Adam" to the per-step code (_set_hyper, which renews it and _opt_hyper for the other kinds; one attribute to read)
        self._opt_key = self.optimizer.hyper_key()
        assert (self._opt_key is None) == (self.optimizer.kind == N.OPT_ADAM)
        # (Adam through the general entry points: the kind alone, its hyper-parameters stay in prism_learner_desc.hyper)
        self._opt_hyper = self.optimizer.native_hyper()
        if self._opt_hyper is None and self._opt_calls:
            self._opt_hyper = N.OptHyper(N.OPT_ADAM, 0.0, 0.0, 0.0)
        self.dims = model_dims(config, in_channels, n_actions)
        self.off = _offsets(model)
        # prism_act_forward fills a Q-value array: two-layer heads (forward tiles) or single-Linear heads (a workgroup per row)
        self._act_q = self.dims.n_heads > 0 and self.dims.head_layers in (1, 2)
        self.tau_rng = getattr(config, "tau_rng", "philox")
        self.overlap_writeback = bool(getattr(config, "overlap_writeback", True))
        self.seed = int(config.seed)
        self._draw_offset = 0      # tau counters consumed by update() (host-issued offsets)
        self._fused_tau = 0        # ... and by fused steps (device counter, mirrored: one counter space for both paths)
        self._act_draws = 0        # acting draws: a Philox stream of their own (key 3), counted separately
        self._act_raw = None
        self.pg = process_group
        self.world = 1
        if process_group is not None or (torch.distributed.is_available() and torch.distributed.is_initialized()
                                         and getattr(config, "data_parallel", False)):
            self.world = torch.distributed.get_world_size(process_group)
        self._B = None
        # the all-reduce captured INSIDE the step graph: opt-in (config.collective_in_graph / PRISM_COLLECTIVE_IN_GRAPH=1)
        # until a multi-GPU run of it is on record; the default is two graphs around an eagerly launched collective
        self.collective_in_graph = bool(getattr(config, "collective_in_graph",
                                                os.environ.get("PRISM_COLLECTIVE_IN_GRAPH", "0") == "1"))
        # the fused tail's grid barrier needs the launch resident at once, which the library can only prove for a GPU this
        # process has to itself: PRISM_SHARED_GPU=1 (several learners per GPU, a normal MinAtar set-up) switches it off
        self.fuse_tail = bool(getattr(config, "fuse_tail", os.environ.get("PRISM_SHARED_GPU", "0") != "1"))
        self._status = pdist.StatusWords()        # pinned host mirror of the sticky status bits: polled every step
        # Agent.forward replayed from one hipGraph per (number of observations, selector): H2D of the observations, embed,
        # forward tiles, selector kernel, D2H of the actions (config.act_graph = False: the eager launches)
        self.act_graph = bool(getattr(config, "act_graph", True))
        self.fill_graph_replays = 0               # replays of the cursor-form step graph (step_fused fill_graph; tests, tools)
        # epsilon-greedy with one coin per observation, tossed on the device (prism_egreedy_select), where the default tosses
        # the reference's one host coin per call.  The position of that stream is the selector's epsilon.current_step; the
        # device keeps a copy (_eg_word) that captured calls advance, _eg_dev_steps is what the host knows it to hold
        self.e_greedy_per_env = bool(getattr(config, "e_greedy_per_env", False))
        self._eg_word, self._eg_dev_steps = None, None
        # risk-sensitive acting (config.iqn_risk_policy_id, agents/risk_policies.py): (PRISM_RISK_* id, eta).  Non-neutral:
        # every acting forward embeds beta(tau) -- one prism_act_tau_distort in front of it (_act_launch); the update stays
        # neutral.  Neutral: no launch, no buffer, the keys and records of an agent without the knob
        from prism_amd.agents import risk_policies
        self.risk = risk_policies.for_config(config)
        self._risk_on = self.risk[0] != N.RISK_NEUTRAL
        self._param_epoch, self._act_packed_at = 0, None
        # (the reference's async evaluator loads weights straight into agent.model, async_agent_evaluator.py:29)
        self.model.register_load_state_dict_post_hook(lambda module, incompatible: self._params_replaced())
        self._capture_error = None
        # the step's one exchange: "rccl" (torch.distributed all_reduce, the default) or "direct" (two shots over peer-mapped
        # buffers, prism_amd/dist.py DirectAllReduce)
        self.collective = str(getattr(config, "collective", "rccl"))
        self._direct = None
        if self.world > 1 and self.collective == "direct":
            self._direct = pdist.DirectAllReduce(self.grads, self.pg, status=self._status)
            if not self._direct.use_flags:
                self.collective_in_graph = False          # host-side barriers cannot be captured
        self.model.train()

    def _allreduce(self):
        if self._direct is not None:
            return self._direct.allreduce(self.grads)
        return pdist.allreduce_grads(self.grads, self.pg)

    # ------------------------------------------------------------------ descriptor
    def _prepare(self, B):
        L = N.lib()
        rc = L.prism_learner_supported(ctypes.byref(self.dims), B)
        if rc != N.PRISM_OK:
            from prism_amd.factory.model_factory import UnsupportedConfig
            raise UnsupportedConfig(
                f"prism_amd HIP learner does not cover this configuration at batch {B} "
                f"(use_iqn={self.dims.use_iqn}, n_heads={self.dims.n_heads}, layer_norm={self.dims.use_layer_norm}, "
                f"T={self.dims.n_tau}); there is no eager fallback")
        dev = self.device
        ws_bytes = L.prism_learner_workspace_bytes(ctypes.byref(self.dims), B)
        self.workspace = torch.zeros((ws_bytes + 3) // 4, dtype=torch.float32, device=dev)
        self.out_dl = torch.zeros(B, device=dev)
        self.out_ql = torch.zeros(B, device=dev)
        self.out_td = torch.zeros(B, device=dev)
        self.scalars = torch.zeros(8, device=dev)
        maxT = max(self.dims.n_tau, self.dims.n_tau_next)
        self.tau_out = torch.zeros(3, maxT * B, device=dev)
        self.ones_w = None
        d = N.LearnerDesc()
        d.dims, d.off, d.batch = self.dims, self.off, B
        d.gemm_mode = N.GEMM_MODES[str(getattr(self.config, "gemm_mode", "auto"))]      # "fp32" | "bf16x3" | "auto"
        d.params, d.grads = self.flat.data_ptr(), self.grads.data_ptr()
        d.target_params = self.flat_target.data_ptr() if self.flat_target is not None else None
        d.adam_m, d.adam_v = [t.data_ptr() for t in self.optimizer.native_buffers()]
        d.adam_step = self.optimizer.step_t.data_ptr()
        d.tau_out = self.tau_out.data_ptr()
        d.out_dist_loss, d.out_q_loss = self.out_dl.data_ptr(), self.out_ql.data_ptr()
        d.out_td, d.out_scalars = self.out_td.data_ptr(), self.scalars.data_ptr()
        d.workspace, d.workspace_bytes = self.workspace.data_ptr(), ws_bytes
        d.host_status = self._status.data_ptr()
        if self._direct is not None:      # a collective that gives up poisons THIS workspace's status word (no update applied)
            self._direct._desc.poison = self.workspace.data_ptr() + 4 * N.WS_STATUS_WORD
        self.rng_counters = torch.zeros(3, dtype=torch.int64, device=dev)     # {PER draws, tau draws, acting draws}
        self._rng_ptr = self.rng_counters.data_ptr()
        self._act_graphs, self._act_ptrs, self._act_dev_draws, self._act_packed_at = {}, {}, 0, None
        self._act_slots = {}          # estimate buffers of acting passes enqueued into a caller's capture (_enqueue_act)
        self._eg_word, self._eg_dev_steps = torch.zeros(1, dtype=torch.int64, device=dev), None
        # observations one prism_act_forward takes: what the workspace holds, in whole 16-row tiles for two-layer Q heads
        self._act_cap = (B // 16) * 16 if self.dims.n_heads > 0 and self.dims.head_layers == 2 else B
        self._desc, self._B = d, B
        self._graphs = {}

    def _set_hyper(self):
        g, h = self.optimizer.param_groups[0], self._desc.hyper
        if self._opt_key is None:
            h.lr, h.beta1, h.beta2, h.eps = g["lr"], g["betas"][0], g["betas"][1], g["eps"]
        else:
            h.lr, h.beta1, h.beta2, h.eps = g["lr"], 0.0, 0.0, 0.0          # (the Adam fields are not read for this kind)
            self._opt_hyper = self.optimizer.native_hyper()
            self._opt_key = self.optimizer.hyper_key()
        h.max_grad_norm, h.grad_scale = self.max_grad_norm, 1.0 / self.world

    def _clip_step(self, d):
        """clip_grad_norm_ + optimizer.step() (agent.py:73-74) on the current stream."""
        L, st = N.lib(), N.current_stream_handle()
        if self._opt_calls:
            N.check(L.prism_learner_clip_step(ctypes.byref(d), ctypes.byref(self._opt_hyper), st), "prism_learner_clip_step")
        else:
            N.check(L.prism_learner_clip_adam(ctypes.byref(d), st), "prism_learner_clip_adam")

    # ------------------------------------------------------------------ reference API
    def update(self, batch, per_weights=1, taus=None):
        """One TD update (agent.py:43-79).  ``taus``: optional explicit quantile samples in the
        reference's draw order (parity tests); otherwise drawn in-kernel (Philox) or with
        ``torch.rand`` when ``config.tau_rng == 'torch'``."""
        self.train()
        if self.world > 1:
            self.poll_status()
        obs = batch["observation"]
        B = int(obs.shape[0])
        if self._B != B:
            self._prepare(B)
        d = self._desc
        nobs, rew = batch["next"]["observation"], batch["next"]["reward"]
        act = batch["action"]
        if act.dim() == 2 and act.shape[-1] != 1:
            act = act.argmax(dim=-1)
        nt = batch["nonterminal"]
        if nt.dtype not in (torch.bool, torch.uint8):      # the kernels read one byte per sample
            nt = nt != 0
        keep = [obs.float().contiguous(), nobs.float().contiguous(), rew.float().contiguous(),
                nt.contiguous(), batch["gamma"].float().contiguous(),
                act.long().contiguous()]
        d.obs, d.next_obs, d.reward, d.nonterminal, d.gamma, d.action = [t.data_ptr() for t in keep]
        if torch.is_tensor(per_weights):
            w = per_weights.to(self.device, torch.float32).contiguous()
            keep.append(w)
            d.per_weights = w.data_ptr()
        else:
            if float(per_weights) != 1.0:
                w = torch.full((B,), float(per_weights), device=self.device)
                keep.append(w)
                d.per_weights = w.data_ptr()
            else:
                d.per_weights = None
        if taus is None and self.tau_rng == "torch" and self.dims.use_iqn:
            T, Tn = self.dims.n_tau, self.dims.n_tau_next
            taus = [torch.rand([T * B, 1], device=self.device)]
            if not self.dims.has_target or self.dims.double_q:
                taus.append(torch.rand([Tn * B, 1], device=self.device))
            if self.dims.has_target:
                taus.append(torch.rand([Tn * B, 1], device=self.device))
        d.tau_cur = d.tau_next_online = d.tau_next_target = None
        if taus is not None and len(taus) > 0 and self.dims.use_iqn:
            ts = [t.to(self.device, torch.float32).reshape(-1).contiguous() for t in taus]
            keep.extend(ts)
            it = iter(ts)
            d.tau_cur = next(it).data_ptr()
            if not self.dims.has_target or self.dims.double_q:
                d.tau_next_online = next(it).data_ptr()
            if self.dims.has_target:
                d.tau_next_target = next(it).data_ptr()
        d.seed = self.seed
        d.offset = self._draw_offset + self._fused_tau
        d.rng_counters, d.embed_done, d.fused_replay, d.fuse_tail = None, 0, None, 0
        self._draw_offset += 3 * max(self.dims.n_tau, self.dims.n_tau_next) * B
        self._set_hyper()
        L = N.lib()
        with torch.cuda.device(self.device):
            N.check(L.prism_learner_fwd_bwd(ctypes.byref(d), N.current_stream_handle()), "prism_learner_fwd_bwd")
            if self.world > 1:
                self._allreduce()
            self._clip_step(d)
        self._keep = keep
        return self._step_done()

    def _step_done(self):
        """What ``update()`` and ``step_fused()`` leave behind for ``log()`` and hand back: the TD errors."""
        self._static_total_loss = self.scalars[0]
        self._static_distribution_loss = self.out_dl if self.dims.use_iqn else None
        self._static_q_loss = self.out_ql if self.dims.n_heads > 0 else None
        self.n_updates += 1
        return self.out_td

    # ------------------------------------------------------------------ fused hot path
    def _bind_fused(self, buf):
        """Point the descriptor at the buffer's static batch / IS weights (stable device addresses)."""
        B = int(buf._index.shape[0])
        if self._B != B:
            self._prepare(B)
        d = self._desc
        d.obs, d.next_obs = buf._obs.data_ptr(), buf._next_obs.data_ptr()
        d.reward, d.nonterminal = buf._reward.data_ptr(), buf._nonterminal.data_ptr()
        d.gamma, d.action = buf._gamma.data_ptr(), buf._action.data_ptr()
        d.per_weights = buf._weight.data_ptr() if buf.use_per else None
        d.tau_cur = d.tau_next_online = d.tau_next_target = None
        d.seed = self.seed
        self._set_hyper()
        return d

    def _launch_fused(self, buf, d, part="all", cursor_slot=None):
        """The step's launches on the current stream.  ``cursor_slot``: None, the front takes the ring's size by value; 0 | 1,
        it reads ``min(cursor[slot], capacity)`` from the buffer's cursor words on the device (prism_step_front_cursor)."""
        L, st = N.lib(), N.current_stream_handle
        rp = ctypes.byref(buf._desc)
        smp = buf.buffer._sampler
        if buf.use_per and self.overlap_writeback:
            d.fused_replay = ctypes.cast(ctypes.pointer(buf._desc), ctypes.c_void_p)
            d.fused_index, d.fused_alpha, d.fused_eps = buf._index.data_ptr(), smp._alpha, smp._eps
        else:
            d.fused_replay = None
        # one GPU, whole step in one go: the gradient reduction rides in prism_step_back's launch (grid barrier)
        # (the fused tail is built for Adam only: the other optimizers run the post + back launch pair)
        d.fuse_tail = int(part == "all" and self.world == 1 and self.fuse_tail and self._opt_key is None)
        if part in ("all", "front"):
            d.embed_done = 1
            if cursor_slot is not None:
                N.check(L.prism_step_front_cursor(ctypes.byref(d), rp, buf._ring_kind, N.ptr(buf._cursor_words), cursor_slot,
                                                  None, buf.seed, buf._draws, buf.buffer._sampler._beta, N.ptr(buf._index),
                                                  N.ptr(buf._weight), st()), "prism_step_front_cursor")
            elif buf._ring_kind:                           # a byte ring: the same launch, its row loads a word per thread
                N.check(L.prism_step_front_ring(ctypes.byref(d), rp, buf._ring_kind, buf._size, None, buf.seed, buf._draws,
                                                buf.buffer._sampler._beta, N.ptr(buf._index), N.ptr(buf._weight), st()),
                        "prism_step_front_ring")
            else:
                N.check(L.prism_step_front(ctypes.byref(d), rp, buf._size, None, buf.seed, buf._draws,
                                           buf.buffer._sampler._beta, N.ptr(buf._index), N.ptr(buf._weight), st()),
                        "prism_step_front")
            N.check(L.prism_learner_fwd_bwd(ctypes.byref(d), st()), "prism_learner_fwd_bwd")
            d.embed_done = 0
        if part == "all" and self.world > 1:
            self._allreduce()
        if part in ("all", "back"):
            if self._opt_calls:
                N.check(L.prism_step_back_opt(ctypes.byref(d), ctypes.byref(self._opt_hyper), rp, N.ptr(buf._index), smp._alpha,
                                              smp._eps, st()), "prism_step_back_opt")
            else:
                N.check(L.prism_step_back(ctypes.byref(d), rp, N.ptr(buf._index), smp._alpha, smp._eps, st()),
                        "prism_step_back")

    def step_fused(self, buf, eager=False, use_graph=True, fill_graph=False):
        """Sample + update + priority writeback as four launches on one GPU, five around an all-reduce (prism_step_front, fwd_bwd,
        prism_step_back); replayed from a hipGraph when the replay is full (its size is baked into
        the captured launches) and the RNG counters live on the device.  ``fill_graph`` (the learner passes its
        ``graph_while_filling``, the one place the knob is held): while the ring is still filling, replay the form whose front
        reads the ring's size from the buffer's cursor words instead (``fill_form``); at the fill the step goes over to the
        by-value graph."""
        d = self._fused_begin(buf)
        slot = None
        if use_graph and not eager and fill_graph and buf._size < buf.capacity and self.fill_form(buf) is None:
            slot = buf._cursor_known[0] if buf._cursor_known is not None else 0
        graphable = use_graph and not eager and (buf._size == buf.capacity or slot is not None)
        with torch.cuda.device(self.device):
            if not graphable:
                self._launch_fused(buf, d)
            else:
                key = self._fused_key(buf, d, slot)
                g = self._graphs.get(key)
                if slot is not None:
                    buf.seed_cursor(slot)                       # an eager ingest, a bulk load or a restore moved the count
                if g is None:
                    self._graphs.clear()                        # arguments changed: older captures are stale
                    self._launch_fused(buf, d, cursor_slot=slot)   # first step of a form runs eagerly
                    self._graphs[key] = "warm"
                elif g == "warm":
                    torch.cuda.current_stream().synchronize()
                    self._graphs[key] = self._capture(buf, d, slot)   # capture, then replay once = this step
                else:
                    g[0].replay()
                    if slot is not None:
                        self.fill_graph_replays += 1
                    if len(g) == 2:          # data parallel, two graphs around an eagerly launched collective
                        self._allreduce()
                        g[1].replay()
        return self._fused_mirror(buf)

    def fill_form(self, buf):
        """Why the step cannot run in the form that reads the ring's size from the device (None: it can)."""
        if self.world != 1:
            return "data parallel (world > 1) keeps the step eager until the ring is full"
        if self.tau_rng != "philox" or buf.mass_rng != "philox":
            return "tau_rng and per_mass_rng must be 'philox'"
        if buf._desc is None or buf._size != min(buf._serial, buf.capacity):
            return ("the ring's write serial is behind its size (a load in the reference's format): the step stays eager "
                    "until the ring is full")
        return None

    def _fused_begin(self, buf):
        """What every fused step does on the host before its launches: the sticky bits polled, the descriptor bound to the
        buffer's static batch and to the device counters.  Returns the descriptor."""
        if self.tau_rng != "philox" or buf.mass_rng != "philox":
            raise RuntimeError("fused step draws its random numbers in-kernel (per_mass_rng/tau_rng = 'philox')")
        if buf._index is None or buf._index.shape[0] != buf.buffer._batch_size:
            buf._alloc_batch(buf.buffer._batch_size)
        self.poll_status()
        d = self._bind_fused(buf)
        d.rng_counters = self._rng_ptr
        d.offset = self._draw_offset               # device counter + what update() has consumed: never the same draw twice
        return d

    def _fused_key(self, buf, d, form=None):
        """Everything a captured ``_launch_fused`` bakes by value: hyper-parameters, seeds, beta / alpha, offsets -- and the
        ring's size, or what stands for it in the cursor form: ``form`` (the step graph: the slot of the word that holds the
        size; the captured iteration: ``CURSOR_FORM``, its two graphs bake one slot each)."""
        h, smp = d.hyper, buf.buffer._sampler
        return (id(buf), buf._size if form is None else ("cursor", form), self.world, h.lr, h.beta1, h.beta2,
                h.eps, h.max_grad_norm, h.grad_scale, self._opt_key, self.seed, buf.seed, smp._beta, smp._alpha, smp._eps,
                self._draw_offset, buf._draws, self.overlap_writeback)

    def _fused_mirror(self, buf):
        """The host mirrors of one fused step that ran (eagerly, from the step graph, or inside a larger replay): the two
        device draw counters and what ``_step_done`` keeps.  Returns the TD errors."""
        self._fused_tau += 3 * max(self.dims.n_tau, self.dims.n_tau_next) * self._B
        buf._fused_draws += self._B
        return self._step_done()

    def _capture(self, buf, d, cursor_slot=None):
        if self.world == 1:
            g = torch.cuda.CUDAGraph()
            with graph_capture(g):
                self._launch_fused(buf, d, cursor_slot=cursor_slot)
            g.replay()
            return (g,)
        if self.collective_in_graph:
            # data parallel, one graph: front + forward/backward, the RCCL all-reduce of the flat gradient, clip + Adam
            # + writeback -- one launch per step, no host round trip around the collective.  The collective must have run
            # once eagerly (communicator set up outside the capture): the warm step before this one did that.  Backends
            # whose all-reduce cannot be captured (gloo: host staging) raise here; the step then falls back to two
            # graphs around an eagerly launched collective, for good.
            g, err = torch.cuda.CUDAGraph(), None
            try:
                with graph_capture(g, capture_error_mode="thread_local"):
                    self._launch_fused(buf, d)
            except Exception as e:          # noqa: BLE001 -- any capture failure selects the split form
                err = repr(e)
                torch.cuda.synchronize()
            # every rank must run the same form: agree on the outcome (MIN over ranks of "my capture worked")
            ok = torch.tensor([0 if err else 1], device=self.device, dtype=torch.int32)
            torch.distributed.all_reduce(ok, op=torch.distributed.ReduceOp.MIN, group=self.pg)
            if int(ok.item()) == 1:
                g.replay()
                return (g,)
            self.collective_in_graph = False
            self._capture_error = err or "capture failed on another rank"
            import warnings
            warnings.warn(f"prism_amd: the all-reduce could not be captured into the step graph ({self._capture_error}); "
                          "running two graphs around an eager collective")
            # nothing of the step has run yet (a capture only records): fall through
        g1, g2 = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
        with graph_capture(g1):
            self._launch_fused(buf, d, "front")
        g1.replay()
        self._allreduce()
        with graph_capture(g2):
            self._launch_fused(buf, d, "back")
        g2.replay()
        return (g1, g2)

    # ------------------------------------------------------------------ acting
    def _act_T(self):
        """Quantile samples per action of one acting forward (composite_model.py:57): its draws are ``T * n``."""
        return int(self.model.distribution_model.n_quantile_samples_per_action) if self.dims.use_iqn else 0

    @contextlib.contextmanager
    def acting_stream(self, offset):
        """The calls inside draw their acting samples (quantile draws, the sampled selector's draw: key ``TAU_KEY + TAU_ACT``
        and ``"IDSA"``) at draw count ``offset`` onwards instead of the agent's own; afterwards the count is what it was, so
        the calls that follow draw what they would have drawn without the block (the device's word follows at the next
        graph call, as after any eager call: ``_forward_graph``).  Hands back an object whose ``count`` is the count the
        block reached -- where a later block goes on.  An evaluation runs in one (prism_amd/evals.py)."""
        offset = int(offset)
        if not 0 <= offset < 2 ** 63:
            raise ValueError("acting_stream: the offset is a draw count in [0, 2^63)")
        reached = _DrawCount(offset)
        keep = self._act_draws
        self._act_draws = offset
        try:
            yield reached
        finally:
            reached.count = self._act_draws
            self._act_draws = keep

    def _act_buffers(self, n):
        """``(z, qb, n_pad, T)``: the estimate arrays ``prism_act_forward`` fills for ``n`` observations and the selector
        kernels read -- quantile values ``z[T*n (padded to whole 16-row tiles), A]`` with IQN, Q values
        ``qb[heads, n_pad, A]`` with Q heads, None for what the model does not have."""
        dm, T = self.dims, self._act_T()
        n_pad = (n + 15) // 16 * 16
        z = torch.empty(((n * T + 15) // 16 * 16, dm.n_actions), device=self.device) if dm.use_iqn else None
        qb = torch.empty((dm.n_heads, n_pad, dm.n_actions), device=self.device) if self._act_q else None
        return z, qb, n_pad, T

    def _risk_buffer(self, n, T):
        """Where ``prism_act_tau_distort`` leaves the distorted samples of an acting pass of ``n`` observations (None for
        a neutral agent: no launch, no buffer).  A capture bakes its address: one per capturing slot, beside ``z``."""
        return torch.empty(n * T, device=self.device) if self._risk_on and T > 0 else None

    def _act_launch(self, obs, n, T, tau, offset, z, qb, rng_counters, act_flags, risk_tau=None):
        """The one ``prism_act_forward`` call, on the current stream.  The caller says who counts the draws, never the
        descriptor as the last learner step left it: a fused step leaves it pointing at the device counters (step_fused),
        and with them set ``prism_act_forward`` adds ``rng_counters[2]`` to ``offset`` and advances it.  That word belongs
        to the graph path (_forward_graph: ``rng_counters`` bound, offset 0), which seeds it from ``_act_draws`` whenever
        an eager call has moved the count on; the eager call (act_estimates) draws at the HOST's count (``rng_counters``
        None, offset ``_act_draws``) and has the packed weight copies rebuilt (``act_flags`` 0).  Both fields go back to
        what they were.  A capture bakes every argument: ``obs``, ``z``, ``qb`` are the capturing slot's own buffers.
        With a risk policy one ``prism_act_tau_distort`` runs first: it draws the raw samples where the forward would have
        (or takes ``tau`` as the raw ones), advances the device word when it is bound, and leaves beta of them in
        ``risk_tau`` (_risk_buffer), which the forward then takes as explicit samples with the word unbound."""
        d = self._desc
        if self._risk_on:
            N.check(N.lib().prism_act_tau_distort(n, T, self.risk[0], self.risk[1], N.ptr(tau), self.seed, offset, rng_counters,
                                                  N.ptr(risk_tau), None, N.current_stream_handle()), "prism_act_tau_distort")
            tau, rng_counters = risk_tau, None
        keep = d.rng_counters, d.act_flags
        d.rng_counters, d.act_flags = rng_counters, act_flags
        try:
            N.check(N.lib().prism_act_forward(ctypes.byref(d), N.ptr(obs), n, T, N.ptr(tau), self.seed, offset, N.ptr(z),
                                              N.ptr(qb), N.current_stream_handle()), "prism_act_forward")
        finally:
            d.rng_counters, d.act_flags = keep

    _SCORED = ("ids", "ids_sampled", "min_regret", "simple_ids")          # selector kernels that leave (n, A) scores behind

    def _selector_key(self, sel):
        """``_kernel_key`` of the selector, with ``("risk", policy id, eta)`` behind it for an agent that acts under a risk
        policy: every graph keyed by it (the acting graphs, the captured iteration) bakes the policy's launch."""
        key = self._kernel_key(sel)
        return key if key is None or not self._risk_on else key + (("risk",) + self.risk,)

    def _kernel_key(self, sel):
        """The selector's native kernel and constants: ``("ids", lmbda, epsilon, rho_lower_bound, unsquish id)``,
        ``("ids_sampled", ...)`` with the same constants for ``ids_use_random_samples`` (the action is a Philox draw of the
        agent's seed: only where the quantile draws are, ``tau_rng == "philox"``), ``("greedy",)``,
        ``("min_regret", lmbda, unsquish id)`` and ``("simple_ids", beta, unsquish id)`` for the two selectors that read the
        ensemble alone (``prism_min_regret_select`` / ``prism_simple_ids_select``; a model with Q heads),
        ``("egreedy", start, stop, max_steps)`` for epsilon-greedy per observation (``e_greedy_per_env``; ``forward`` hands
        the selector over only in that mode, else its ``greedy`` member), or None for what has
        none (sampled IDS in parity mode -- ``torch.multinomial`` on torch's generator --, an unsquish function the kernel
        does not know, IDS on a model without both estimate arrays, any other selector): the selector's torch code on the
        eager estimates."""
        from prism_amd.agents.action_selectors import (EGreedyActionSelector, GreedyActionSelector, IDSActionSelector,
                                                       MinRegretActionSelector, SimpleIDSActionSelector)
        if type(sel) is EGreedyActionSelector and self.e_greedy_per_env:
            e = sel.epsilon
            if int(e.max_steps) != e.max_steps or e.max_steps < 0 or e.current_step < 0:
                raise ValueError("e_greedy_per_env counts rows: the anneal needs a whole, non-negative number of steps")
            return ("egreedy", float(e.start), float(e.stop), int(e.max_steps))
        if type(sel) is IDSActionSelector:
            from prism_amd.agents.squish_functions import unsquish_id
            usq = unsquish_id(sel.unsquish_function)
            if usq is None or not (self.dims.use_iqn and self._act_q) or (sel.random_sample and self.tau_rng != "philox"):
                return None
            return ("ids_sampled" if sel.random_sample else "ids", float(sel.lmbda), float(sel.epsilon),
                    float(sel.ids_rho_lower_bound), usq)
        if type(sel) in (MinRegretActionSelector, SimpleIDSActionSelector):
            from prism_amd.agents.squish_functions import unsquish_id
            usq = unsquish_id(sel.unsquish_function)
            if usq is None or not self._act_q or self.dims.n_heads > 16:
                return None
            if type(sel) is MinRegretActionSelector:
                return None if self.dims.n_heads < 2 else ("min_regret", float(sel.lmbda), usq)
            return None if sel.random_sample else ("simple_ids", float(sel.beta), usq)
        return ("greedy",) if type(sel) is GreedyActionSelector else None

    def _select_launch(self, skey, z, qb, n, n_pad, T, act, host_act, scores, draw_offset=0, rng_counters=None,
                       eg_rows=None, eg_word=None):
        """The selector kernel of ``skey`` (_selector_key) on the current stream: actions to ``act`` (device) and, where
        given, to ``host_act`` (pinned host); ``scores``: the ``(n, A)`` information ratios IDS leaves behind (MinRegret: the
        squared regrets, SimpleIDS: the scaled values).  Sampled
        IDS draws observation b at Philox counter c0 + b, c0 the acting count at the START of this call's forward: the
        eager call hands it over (``draw_offset``), the graph path binds ``rng_counters``, whose word [2] the forward in
        front of this launch has advanced by n * T (the kernel takes that off again).  Epsilon-greedy per observation
        draws row b at counter s0 + row0 + b, s0 the rows seen before this call: the eager call hands over
        ``eg_rows = (s0, row0, rows of the whole call)``, the graph path binds ``eg_word``, the device's own count, which
        the launch advances."""
        L, dm = N.lib(), self.dims
        if skey[0] == "egreedy":
            s0, row0, n_call = eg_rows if eg_word is None else (0, 0, n)
            N.check(L.prism_egreedy_select(N.ptr(z), N.ptr(qb), n, n_pad, T, dm.n_actions, dm.n_heads, skey[1], skey[2], skey[3],
                                           self.seed, s0, row0, n_call, eg_word, None, None, None, None, N.ptr(act),
                                           N.ptr(host_act), N.current_stream_handle()), "prism_egreedy_select")
            return
        if skey[0] == "min_regret":
            N.check(L.prism_min_regret_select(N.ptr(qb), n, n_pad, dm.n_actions, dm.n_heads, skey[1], skey[2], N.ptr(scores),
                                              None, N.ptr(act), N.ptr(host_act), N.current_stream_handle()),
                    "prism_min_regret_select")
            return
        if skey[0] == "simple_ids":
            N.check(L.prism_simple_ids_select(N.ptr(qb), n, n_pad, dm.n_actions, dm.n_heads, skey[1], skey[2], N.ptr(scores),
                                              None, N.ptr(act), N.ptr(host_act), N.current_stream_handle()),
                    "prism_simple_ids_select")
            return
        if skey[0] == "ids_sampled":
            N.check(L.prism_ids_sample_select(N.ptr(z), N.ptr(qb), n, n_pad, T, dm.n_actions, dm.n_heads, skey[1], skey[2],
                                              skey[3], skey[4], None, self.seed, draw_offset, rng_counters, N.ptr(scores), None,
                                              None, N.ptr(act), N.ptr(host_act), N.current_stream_handle()),
                    "prism_ids_sample_select")
            return
        if skey[0] == "ids":
            N.check(L.prism_ids_select(N.ptr(z), N.ptr(qb), n, n_pad, T, dm.n_actions, dm.n_heads, skey[1], skey[2], skey[3],
                                       skey[4], N.ptr(scores), None, N.ptr(act), N.ptr(host_act), N.current_stream_handle()),
                    "prism_ids_select")
        else:
            N.check(L.prism_greedy_select(N.ptr(z), N.ptr(qb), n, n_pad, T, dm.n_actions, dm.n_heads, N.ptr(act), None,
                                          N.ptr(host_act), N.current_stream_handle()), "prism_greedy_select")

    @torch.no_grad()
    def act_estimates(self, obs, taus=None):
        """``(q_estimates, return_distribution)`` as ``CompositeModel.forward(x, for_action=True)`` hands them to the
        action selector (composite_model.py:51-70): ``(n, A, heads)`` and ``(n_quantile_samples_per_action, n, A)``,
        computed by ``prism_act_forward`` on the learner's flat parameters (forward tiles for the IQN rows and the
        two-layer heads, one workgroup per observation for the single-Linear DQN head).  ``taus``: explicit quantile
        samples ``[T*n, 1]`` in the reference's order (parity tests)."""
        from prism_amd.agents.modules import _as_tensor
        obs = _as_tensor(obs, self.device).contiguous()
        if self._B is None:
            self._prepare(int(self.config.batch_size))
        n, A, cap = int(obs.shape[0]), self.dims.n_actions, self._act_cap
        if cap < 1:
            raise ValueError(f"acting through the Q-head tiles needs a learner batch of at least 16 (batch {self._B})")
        if n > cap:          # more observations than the learner's workspace holds at once: in pieces
            parts = [self.act_estimates(obs[i:i + cap], None if taus is None else
                                        taus.view(-1, n)[:, i:i + cap].reshape(-1, 1)) for i in range(0, n, cap)]
            q = torch.cat([p[0] for p in parts], dim=0) if parts[0][0] is not None else None
            dist = torch.cat([p[1] for p in parts], dim=1) if parts[0][1] is not None else None
            self._act_raw = None          # (describes the last piece only: nobody may select from it)
            return q, dist
        z, qb, n_pad, T = self._act_buffers(n)
        if taus is None and self.dims.use_iqn and self.tau_rng == "torch":
            taus = torch.rand([T * n, 1], device=self.device)
        tau = None if taus is None else taus.to(self.device, torch.float32).reshape(-1).contiguous()
        with torch.cuda.device(self.device):          # at the host's acting count, packed weight copies rebuilt
            self._act_launch(obs, n, T, tau, self._act_draws, z, qb, rng_counters=None, act_flags=0,
                             risk_tau=self._risk_buffer(n, T))
        self._act_draws += T * n
        self._act_raw = (z, qb, n, n_pad, T)
        dist = z[:n * T].view(n, T, A).permute(1, 0, 2) if z is not None else None
        if qb is not None:
            q = qb[:, :n].permute(1, 2, 0)
        else:
            # models without Q heads (composite_model.py:66-68); the native selectors below take this mean from z themselves
            q = dist.mean(dim=0).unsqueeze(-1)
        return q, dist

    @torch.no_grad()
    def forward(self, obs):
        """Agent.forward (agent.py:31-41).  Minimum-regret and simple-IDS selection on the ensemble
        (``prism_min_regret_select``, ``prism_simple_ids_select``), information-directed sampling, deterministic
        (``prism_ids_select``) and sampled
        (``ids_use_random_samples``: ``prism_ids_sample_select``, the action a Philox draw of the agent's seed on its own
        stream key), greedy and epsilon-greedy selection (``prism_greedy_select``; the coin and the random actions come from
        the selector's host generator exactly as in action_selectors.py:35-45; with ``config.e_greedy_per_env`` every
        observation has its own coin and random action, Philox draws inside ``prism_egreedy_select``, the selector's
        ``epsilon.current_step`` the position of that stream and its ``rng`` left alone) run natively on the estimate
        buffers.  Only in
        parity mode (``tau_rng == "torch"``) sampled IDS runs the selector's torch code: ``torch.multinomial`` on torch's
        generator, as the reference draws."""
        from prism_amd.agents.action_selectors import EGreedyActionSelector
        from prism_amd.agents.modules import _as_tensor
        sel = self.eval_action_selector if self._is_eval else self.action_selector
        obs_in = obs
        n, A = int(np.shape(obs)[0]), self.dims.n_actions
        per_env = self.e_greedy_per_env and type(sel) is EGreedyActionSelector
        if type(sel) is EGreedyActionSelector and not per_env:
            if sel.rng.uniform(0, 1) < sel.epsilon.update(n):       # one coin for the whole call (action_selectors.py:38-41)
                # the reference has ALREADY run the model by the time it tosses the coin (agent.py:33 -> :36): the forward's
                # quantile samples are drawn whether or not the estimates are used.  The estimates are not needed here, the
                # draws are: consume them, so that every later greedy action sees the stream it would see in the reference
                if self.dims.use_iqn:
                    T = self._act_T()
                    if self.tau_rng == "torch":
                        torch.rand([T * n, 1], device=self.device)
                    else:
                        self._act_draws += T * n
                return torch.as_tensor(sel.rng.randint(A, size=(n,)), dtype=torch.long).to(self.device)
            sel = sel.greedy
        if self._B is None:
            self._prepare(int(self.config.batch_size))
        cap = self._act_cap
        if n <= cap and self.act_graph and self.tau_rng == "philox":
            out = self._forward_graph(obs_in, n, sel)
            if out is not None:
                return out
        obs = _as_tensor(obs, self.device).contiguous()
        if n > cap:          # in pieces: every piece is selected from its own estimate buffers
            out = torch.cat([self._forward_piece(obs[i:i + cap], sel, i, n) for i in range(0, n, cap)])
        else:
            out = self._forward_piece(obs, sel, 0, n)
        if per_env:
            sel.epsilon.current_step += n          # (the device's count is behind now: the next graph call seeds it)
        return out

    def _forward_graph(self, obs_in, n, sel):
        """One ``Agent.forward`` as ONE hipGraph launch: [observations host -> device] -> prism_act_forward -> selector kernel
        -> [actions device -> pinned host].  Keyed by everything a capture bakes: the number of observations, where they come
        from (the caller's device tensor by address -- the reference's collector reuses one inference buffer,
        experience_collector.py:77-78 -- or the pinned staging block for host arrays), the selector and its constants.  The
        quantile draws come from the device counter ``rng_counters[2]`` (include/prism_hip.h), which mirrors ``_act_draws``.
        Returns None for selectors that have no native kernel (the caller runs the eager path)."""
        skey = self._selector_key(sel)
        if skey is None:
            return None
        dm = self.dims
        shape = (n, 10, 10, dm.in_channels)
        if torch.is_tensor(obs_in) and obs_in.is_cuda and not (obs_in.dtype == torch.float32 and obs_in.is_contiguous()
                                                               and obs_in.numel() == n * 100 * dm.in_channels):
            obs_in = obs_in.float().contiguous().view(shape)          # (a device tensor in another layout: one eager copy)
        on_host = not (torch.is_tensor(obs_in) and obs_in.is_cuda)
        mode = "host" if on_host else "ptr"
        if mode == "ptr":
            # a device tensor is read in place while its address repeats (the collector's one inference buffer); a caller
            # that hands over a fresh tensor every time gets one device-to-device copy into a staging block instead of a
            # capture per address
            seen = self._act_ptrs.setdefault((n, skey), set())
            seen.add(obs_in.data_ptr())
            if len(seen) > 3:
                mode = "dev"
        # the packed weight copies in the workspace follow the parameters: rebuilt by the first acting call after every update
        current = self._act_packed_at == self._param_version()
        key = (n, skey, mode, obs_in.data_ptr() if mode == "ptr" else None, self.seed, self._B, current)
        st = self._act_graphs.get(key)
        if st is None:
            if len(self._act_graphs) > 32:
                self._act_graphs.clear()
            z, qb, n_pad, T = self._act_buffers(n)
            dev = self.device
            st = dict(T=T, n_pad=n_pad, z=z, qb=qb, rtau=self._risk_buffer(n, T), calls=0, g=None,
                      pin_in=[torch.zeros(shape, dtype=torch.float32).pin_memory() for _ in range(4)] if on_host else None,
                      obs=obs_in if mode == "ptr" else (None if on_host else torch.empty(shape, dtype=torch.float32, device=dev)),
                      scores=torch.empty((n, dm.n_actions), device=dev) if skey[0] in self._SCORED else None,
                      act=[torch.empty(n, dtype=torch.int64, device=dev) for _ in range(4)],
                      pin_out=[torch.zeros(n, dtype=torch.int64).pin_memory() for _ in range(4)],
                      ev=[torch.cuda.Event() for _ in range(4)])
            if st["pin_in"] is not None:
                st["pin_np"] = [t.numpy() for t in st["pin_in"]]
            self._act_graphs[key] = st
        self._seed_act_words(skey, sel)          # eager calls / an explore branch moved the host count on
        k = st["calls"] & 3
        if on_host:
            if st["calls"] >= 4:
                st["ev"][k].synchronize()          # the launch that last read this staging slot (four calls ago) is through
            if torch.is_tensor(obs_in):
                st["pin_in"][k].copy_(obs_in.reshape(shape))
            else:
                st["pin_np"][k][...] = np.asarray(obs_in, dtype=np.float32).reshape(shape)
        elif mode == "dev":
            st["obs"].copy_(obs_in.view(shape))

        def launch(slot):
            # (host arrays: the embed kernel reads the pinned staging block in place -- 400 C bytes per observation over the
            # host link cost less than a copy node in front of it; the selector writes the actions to device AND pinned host)
            self._act_launch(st["pin_in"][slot] if on_host else st["obs"], n, st["T"], None, 0, st["z"], st["qb"],
                             rng_counters=self.rng_counters.data_ptr(),
                             act_flags=N.ACT_WEIGHTS_CURRENT if current else 0, risk_tau=st["rtau"])
            self._select_launch(skey, st["z"], st["qb"], n, st["n_pad"], st["T"], st["act"][slot], st["pin_out"][slot],
                                st["scores"], rng_counters=self.rng_counters.data_ptr(),
                                eg_word=self._eg_word.data_ptr())

        with torch.cuda.device(self.device):
            if st["g"] is None and st["calls"] == 0:
                launch(k)                                   # first call of this shape: eager (also warms the library up)
            else:
                if st["g"] is None:
                    # second call: capture one graph per output slot (a slot is a baked address); a capture only records,
                    # this call's work is the replay below
                    torch.cuda.current_stream().synchronize()
                    st["g"] = []
                    for slot in range(4):
                        g = torch.cuda.CUDAGraph()
                        with graph_capture(g):
                            launch(slot)
                        st["g"].append(g)
                st["g"][k].replay()
            st["ev"][k].record()
        self._act_packed_at = self._param_version()
        st["calls"] += 1
        self._act_draws += st["T"] * n
        self._act_dev_draws = self._act_draws
        if skey[0] == "egreedy":          # (by arithmetic: the launch has added n to the device's count)
            sel.epsilon.current_step += n
            self._eg_dev_steps = sel.epsilon.current_step
        self._act_raw = (st["z"], st["qb"], n, st["n_pad"], st["T"])
        self._act_scores = st["scores"]
        return _Actions.wrap(st["act"][k], st["pin_out"][k], st["ev"][k])

    def _seed_act_words(self, skey, sel):
        """Before a launch that binds the device words: ``rng_counters[2]`` follows ``_act_draws`` and the epsilon-greedy
        word the selector's ``current_step`` whenever an eager call, an explore branch, an evaluation or a loaded checkpoint
        has moved the host's count on (a store on the stream, only then)."""
        if self._risk_on and (self._act_draws & (2 ** 62 - 1)) >= 2 ** N.RISK_COUNT_BITS - 2 ** 28:
            # (prism_act_tau_distort keeps its tickets in bits 42 .. 61 of the word while it runs, include/prism_hip.h)
            raise ValueError(f"acting under a risk policy counts draws as k * 2^62 + c with c < 2^42 - 2^28; the count is "
                             f"{self._act_draws}")
        if self._act_dev_draws != self._act_draws:
            self.rng_counters[2] = self._act_draws
            self._act_dev_draws = self._act_draws
        if skey[0] == "egreedy" and self._eg_dev_steps != sel.epsilon.current_step:
            self._eg_word[0] = int(sel.epsilon.current_step)
            self._eg_dev_steps = sel.epsilon.current_step

    def _act_slot(self, n, skey):
        """The estimate buffers of an acting pass that is enqueued without a graph of its own, per (n, selector)."""
        slots, key = self._act_slots, (n, skey)
        st = slots.get(key)
        if st is None:
            z, qb, n_pad, T = self._act_buffers(n)
            scores = torch.empty((n, self.dims.n_actions), device=self.device) if skey[0] in self._SCORED else None
            st = slots[key] = dict(z=z, qb=qb, n_pad=n_pad, T=T, scores=scores, rtau=self._risk_buffer(n, T))
        return st

    def _enqueue_act(self, obs, act, skey, current):
        """One acting pass, enqueue only (safe inside a stream capture): ``prism_act_forward`` on the contiguous float32
        device observations ``obs`` and the selector kernel of ``skey`` into the device int64 tensor ``act``.  No pinned host
        copy, no graph of its own; the draws come from ``rng_counters[2]`` and the epsilon-greedy rows from the device word,
        exactly as ``_forward_graph`` binds them (``_seed_act_words`` first, outside any capture).  ``current``: the packed
        weight copies are those of the parameters (a pass behind another with no update between).  No host mirror moves:
        ``_act_mirror`` does that, once per pass that ran."""
        n = int(obs.shape[0])
        st = self._act_slot(n, skey)
        ptr = self.rng_counters.data_ptr()
        self._act_launch(obs, n, st["T"], None, 0, st["z"], st["qb"], rng_counters=ptr,
                         act_flags=N.ACT_WEIGHTS_CURRENT if current else 0, risk_tau=st["rtau"])
        self._select_launch(skey, st["z"], st["qb"], n, st["n_pad"], st["T"], act, None, st["scores"], rng_counters=ptr,
                            eg_word=self._eg_word.data_ptr())

    def _act_mirror(self, n, skey, sel):
        """The host mirrors of one enqueued acting pass of ``n`` observations that ran, as ``_forward_graph`` applies them."""
        st = self._act_slot(n, skey)
        self._act_packed_at = self._param_version()
        self._act_draws += st["T"] * n
        self._act_dev_draws = self._act_draws
        if skey[0] == "egreedy":          # (by arithmetic: the launch has added n to the device's count)
            sel.epsilon.current_step += n
            self._eg_dev_steps = sel.epsilon.current_step
        self._act_raw = (st["z"], st["qb"], n, st["n_pad"], st["T"])
        self._act_scores = st["scores"]

    def _forward_piece(self, obs, sel, row0, n_call):
        """Rows ``row0 ..`` of an eager call of ``n_call`` observations: estimates, then the selector on them."""
        self._act_raw = None
        c0 = self._act_draws          # (the acting count this piece's forward starts from: the sampled selector's counter)
        q, dist = self.act_estimates(obs)
        skey = self._selector_key(sel)
        if skey is None:
            return sel.select_action(sel.generate_action_probs(dist, q))
        z, qb, n, n_pad, T = self._act_raw
        action = torch.empty(n, dtype=torch.int64, device=self.device)
        scores = torch.empty((n, self.dims.n_actions), device=self.device) if skey[0] in self._SCORED else None
        with torch.cuda.device(self.device):
            self._select_launch(skey, z, qb, n, n_pad, T, action, None, scores, draw_offset=c0,
                                eg_rows=(int(sel.epsilon.current_step), row0, n_call) if skey[0] == "egreedy" else None)
        if scores is not None:
            self._act_scores = scores
        return action

    def _params_replaced(self):
        self._param_epoch += 1

    def _param_version(self):
        """Changes whenever the online parameters may have: every update, checkpoint load, deserialisation."""
        return (self.n_updates, self._param_epoch)

    def _raise_status(self, bits):
        self._graphs = {}
        if bits & N.WS_STATUS_COLLECTIVE_TIMEOUT:
            # terminal: the sticky slot of the flag array keeps the reduce kernels off, so the bit that keeps clip + Adam off
            # stays where it is, in the workspace and in the pinned mirror -- every later poll raises again
            raise pdist.CollectiveTimeout("prism_amd: the direct all-reduce gave up on a peer; the step that hit it applied no "
                                          "update and the replicas may have diverged -- restore a checkpoint, then "
                                          "reset_collective() on all ranks together")
        self._status.clear()
        if self._B is not None:
            self.workspace.view(torch.int32)[N.WS_STATUS_WORD] = 0
        self.fuse_tail = False
        raise RuntimeError("prism_amd: a fused-tail grid barrier timed out (is the GPU shared with another process?); "
                           "the last steps are incomplete -- restore a checkpoint; fuse_tail is now off")

    def poll_status(self):
        """Raise if a kernel has raised a sticky status bit since the last look: an abandoned fused-tail grid barrier or a
        collective that gave up on a peer.  Reads the pinned host mirror of the bits (``prism_learner_desc.host_status``):
        no device synchronisation, so every ``step_fused`` / ``Learner.step`` calls it -- a failed step surfaces one step
        late at most, not at the next ``log()``."""
        bits = self._status.bits()
        if bits:
            self._raise_status(bits)

    def reset_collective(self):
        """The one way out of a ``CollectiveTimeout``: every rank calls it together (it is a collective call where the
        direct all-reduce is in use).  The direct all-reduce is rebuilt over fresh, zeroed flag arrays and only then are the
        status bits cleared; parameters are the caller's business (restore a checkpoint first: replicas may differ)."""
        torch.cuda.current_stream(self.device).synchronize()
        if self._direct is not None:
            poison = self._direct._desc.poison
            self._direct.close()
            self._direct = pdist.DirectAllReduce(self.grads, self.pg, status=self._status)
            self._direct._desc.poison = poison
        self._status.clear()
        if self._B is not None:
            self.workspace.view(torch.int32)[N.WS_STATUS_WORD] &= ~N.WS_STATUS_COLLECTIVE_TIMEOUT
        self._graphs = {}

    def check_status(self):
        """``poll_status`` plus the device's own words (one D2H sync): the workspace status word and, data parallel with the
        direct collective, the sticky slot of the flag array.  An abandoned grid barrier only happens when the launch was not
        resident at once after all -- other processes' kernels on the same GPU -- and leaves the step that hit it half
        applied; the agent switches the fused tail off for what follows."""
        self.poll_status()
        if self._B is not None:
            bits = int(self.workspace.view(torch.int32)[N.WS_STATUS_WORD].item())
            if bits & (N.WS_STATUS_BARRIER_TIMEOUT | N.WS_STATUS_COLLECTIVE_TIMEOUT):
                self._raise_status(bits)
        if self._direct is not None:
            self._direct.check_status()

    def _target_changed(self):
        """The target parameters were written: its stream-packed copies in the workspace are stale (word 2 of the
        workspace, include/prism_hip.h)."""
        if self._B is not None:
            self.workspace.view(torch.int32)[2] = 0

    @torch.no_grad()
    def sync_target_model(self):
        with torch.cuda.device(self.device):
            N.check(N.lib().prism_sync_target(N.ptr(self.flat_target), N.ptr(self.flat), self.flat.numel(),
                                              N.current_stream_handle()), "prism_sync_target")
            self._target_changed()

    def set_static_batch(self, batch):
        self._static_batch = batch

    def get_static_batch(self):
        return self._static_batch

    def eval(self):
        self.model.eval()
        self._is_eval = True

    def train(self):
        self.model.train()
        self._is_eval = False

    def serialize_model(self):
        return self.flat.tolist() if not list(self.model.buffers()) else \
            [x for v in self.model.state_dict().values() for x in v.flatten().tolist()]

    def deserialize_model(self, values):
        self.flat.copy_(torch.as_tensor(values, dtype=torch.float32))
        self._param_epoch += 1

    def save(self, directory):
        """File layout of agent.py:179-203 (reference checkpoints interchange)."""
        self.check_status()
        path = os.path.join(directory, "agent")
        os.makedirs(path, exist_ok=True)
        torch.save(self.model.state_dict(), os.path.join(path, "model.pt"))
        torch.save(self.optimizer.state_dict(), os.path.join(path, "optimizer.pt"))
        if self.target_model is not None:
            torch.save(self.target_model.state_dict(), os.path.join(path, "target_model.pt"))
        state = {"action_selector": self.action_selector, "n_updates": self.n_updates,
                 "eval_action_selector": self.eval_action_selector, "max_grad_norm": self.max_grad_norm,
                 "use_cuda_graph": self.use_cuda_graph}
        with open(os.path.join(path, "state.pkl"), "wb") as f:
            ref_pickle.dump(state, f)          # class paths as the reference names them: it can load this file

    def load(self, directory):
        path = os.path.join(directory, "agent")
        # load_state_dict copies INTO the existing parameters, i.e. into the flat buffer views
        # (tensor-only files: weights_only refuses anything that would run code on load)
        self.model.load_state_dict(torch.load(os.path.join(path, "model.pt"), map_location=self.device, weights_only=True))
        self.optimizer.load_state_dict(torch.load(os.path.join(path, "optimizer.pt"), map_location=self.device,
                                                  weights_only=True))
        if self.target_model is not None:
            self.target_model.load_state_dict(torch.load(os.path.join(path, "target_model.pt"),
                                                         map_location=self.device, weights_only=True))
        with open(os.path.join(path, "state.pkl"), "rb") as f:
            state = ref_pickle.load(f)         # reference-written files name prism.agents.action_selectors.*
        self._graphs = {}                      # captured graphs bake the hyper-parameters restored here
        self._eg_dev_steps = None              # (the selector loaded below carries its own epsilon.current_step)
        self._param_epoch += 1
        self._target_changed()
        self.action_selector = state["action_selector"]
        self.eval_action_selector = state["eval_action_selector"]
        self.max_grad_norm = state["max_grad_norm"]
        self.n_updates = state["n_updates"]
        self.train()

    # ------------------------------------------------------------------ exact resume (prism_amd/util/snapshot.py)
    def _compat_record(self):
        """What a snapshot must share with the agent it is loaded into: the ``prism_model_dims`` fields, the parameter
        count, the optimizer kind, where the quantile draws come from and -- only when it is not neutral, so that a neutral
        agent's record is what it always was -- the risk policy it acts under."""
        rec = {name: getattr(self.dims, name) for name, _ in N.ModelDims._fields_}
        rec.update(n_params=int(self.flat.numel()), optimizer_kind=int(self.optimizer.kind), tau_rng=str(self.tau_rng))
        if self._risk_on:
            from prism_amd.agents import risk_policies
            rec["risk_policy"] = risk_policies.canonical_id(self.risk)
        return rec

    def _state_part(self):
        """Part ``agent_resume`` of a snapshot: the Philox positions ``save()`` does not write.  The quantile draws of
        ``update()`` and of fused steps share one counter space, so their sum is the position."""
        return dict(n_updates=int(self.n_updates), seed=int(self.seed), tau_rng=str(self.tau_rng),
                    tau_draws=int(self._draw_offset + self._fused_tau), act_draws=int(self._act_draws),
                    optimizer_kind=int(self.optimizer.kind))

    def _check_snapshot(self, manifest):
        from prism_amd.util import snapshot
        stored, mine = (manifest.get("compat") or {}).get("agent"), self._compat_record()
        snapshot.check_compat(stored, mine, "HipAgent.load_state")
        # (a neutral agent's record does not carry the field: a snapshot written under a policy is refused all the same)
        snapshot.check_field("risk_policy", stored.get("risk_policy"), mine.get("risk_policy"), "HipAgent.load_state")

    def _restore_part(self, directory, part):
        self.load(directory)
        self.n_updates, self.seed = int(part["n_updates"]), int(part["seed"])
        self._draw_offset, self._fused_tau = int(part["tau_draws"]), 0
        # the device's acting word is seeded from the host count by the next graph call (_forward_graph)
        self._act_draws, self._act_dev_draws = int(part["act_draws"]), 0
        self._eg_dev_steps = None          # likewise the rows epsilon-greedy per observation has seen (state.pkl has them)
        self._act_raw = None
        self._graphs, self._act_graphs, self._act_ptrs, self._act_packed_at = {}, {}, {}, None
        if self._B is not None:
            self.rng_counters[:2].zero_()          # {PER draws, tau draws} of fused steps: counted in the host offsets now

    def save_state(self, directory):
        """``save(directory)`` (the reference's layout: it can still load ``agent/``) plus part ``agent_resume``: with it
        ``load_state`` puts every random stream of the agent back where it was."""
        from prism_amd.util import snapshot
        return snapshot.write_snapshot(directory, {"agent_resume": self._state_part()},
                                       {"compat": {"agent": self._compat_record()}}, extra=self.save)

    def load_state(self, directory):
        """Restore a ``save_state`` snapshot into an agent built from the same configuration: what follows is bit-identical
        to the run that wrote it.  Other model dimensions, optimizer kind or ``tau_rng`` are refused before anything is
        touched."""
        from prism_amd.util import snapshot
        self._check_snapshot(snapshot.read_manifest(directory))
        parts, _ = snapshot.read_snapshot(directory, ["agent_resume"])
        self._restore_part(directory, parts["agent_resume"])

    @torch.no_grad()
    def log(self, logger):
        self.check_status()
        logger.log_data(data=float(self._static_total_loss), group_name="Report/Losses", var_name="Total Loss")
        if self._static_distribution_loss is not None:
            logger.log_data(data=float(self._static_distribution_loss.mean()), group_name="Report/Losses",
                            var_name="Distribution Loss")
        if self._static_q_loss is not None:
            logger.log_data(data=float(self._static_q_loss.mean()), group_name="Report/Losses", var_name="Q Loss")
        if getattr(logger, "holdout_data", None) is not None:
            idx = np.random.randint(0, logger.holdout_data["observation"].shape[0])
            obs = logger.holdout_data["observation"][idx]
            if obs.shape[0] != 1:
                obs = obs.unsqueeze(0)
            q, dist = self.model(obs)
            self.action_selector.log(logger, dist, q)
        self.model.log(logger)
