"""GPU: centered RMSprop and SGD behind the global-norm clip (prism_learner_clip_step / prism_step_back_opt), the
reference's other two optimizers (agent_factory.py:48-58).

Tolerances: parameters and optimizer state after a step within 2e-6 absolute of torch.optim on the CPU, the bound
tests/test_gpu_learner.py uses for Adam; losses within 1e-5 of the reference's recorded values; where the gradient itself
carries the kink allowance `a` of that test, the parameters carry `s * a` with `s` the update's sensitivity to a gradient
error: lr / rmsprop_epsilon for RMSprop (the bound of d(lr g / avg) / dg), lr for SGD.

The update in isolation, measured on an MI355X against torch 2.10 on the CPU (6 742 parameters, three steps, a real
step of state in front; printed by test_update_in_isolation).  Worst absolute difference, and the same in units in the
last place of the CPU value (large where the value itself is tiny: the parameters include biases of 1e-4):
    RMSprop, unclipped   grad_avg 0 (bit-equal)   square_avg 0 (bit-equal)   parameters 3.7e-9 (256 ulp; 41-115 of 6 742 differ)
    RMSprop, clipped     grad_avg 3.7e-9          square_avg 1.9e-9 (4 ulp)  parameters 7.5e-9 (256 ulp)
    SGD, unclipped       parameters 0 (bit-equal)
    SGD, clipped         parameters 1.9e-9 (65 ulp)
Unclipped, every operation is the same IEEE fp32 operation in the same order, and both state buffers and SGD's parameters
ARE bit-equal.  RMSprop's parameters differ in about 1 % of the elements by one unit of the quotient lr * g / avg: the
operation that differs is the square root -- torch's CPU `sqrt` is a vector-library routine that is not correctly rounded
(one unit low on 0.7 % of random inputs against numpy / float64, measured on the host), the kernel's sqrtf is.  Clipped,
the coefficient itself differs in the last place (the CPU takes the norm of per-tensor norms, the kernel folds block
partials), and every element inherits that."""
import contextlib
import io
import os
import socket

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests.test_gpu_learner import LOSS_TOL, build_hip_agent, to_hip_batch
from tests.test_optimizers import NEW_CASES, swap_optimizer

pytestmark = pytest.mark.gpu
STEP_TOL = 2e-6


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return "cuda:0"


def ulps(x, ref):
    """Worst distance in units in the last place of `ref` (float32 arrays)."""
    x, ref = np.asarray(x, np.float32), np.asarray(ref, np.float32)
    assert np.isfinite(x).all() and np.isfinite(ref).all()
    return float((np.abs(x.astype(np.float64) - ref.astype(np.float64)) / np.spacing(np.abs(ref)).astype(np.float64)).max())


def state_buffers(opt):
    """{torch state name: flat device buffer} of a host optimizer."""
    return dict(zip(opt.state_names, opt.buffers()))


def flat_state(topt, params, name):
    return torch.cat([topt.state[p][name].reshape(-1) for p in params])


# ---------------------------------------------------------------------------------------------- 1. the update alone
@pytest.mark.parametrize("clipped", [False, True], ids=["unclipped", "clipped"])
@pytest.mark.parametrize("name", ["dqn_c2_rmsprop", "dqn_c2_sgd"])
def test_update_in_isolation(dev, name, clipped):
    """A random gradient in the flat gradient buffer -> prism_learner_clip_step, against clip_grad_norm_ +
    torch.optim.{RMSprop, SGD} on the CPU, three consecutive steps, 6 742 parameters (not a multiple of 4).  The entry
    point runs in its data-parallel form (grad_scale = 1/2: the norm partials are then taken from the gradient buffer
    itself, not from what a backward pass left), so the CPU side halves the gradient first -- an exact operation."""
    g = H.load_case("dqn_c2_rmsprop")
    extra = dict(use_rmsprop=False) if name.endswith("sgd") else {}
    cfg, agent = build_hip_agent(g, dev, **extra)
    batch, w, taus = H.case_batch(g, 0)
    agent.update(to_hip_batch(batch, dev), per_weights=w.to(dev))          # binds the descriptor; one real step of state
    torch.cuda.synchronize()
    n = agent.flat.numel()
    assert n % 4 != 0
    params = [p.detach().cpu().clone().requires_grad_(True) for p in agent.model.parameters()]
    if cfg.use_rmsprop:
        topt = torch.optim.RMSprop(params, lr=cfg.learning_rate, alpha=cfg.rmsprop_alpha, eps=cfg.rmsprop_epsilon, centered=True)
    else:
        topt = torch.optim.SGD(params, lr=cfg.learning_rate)
    topt.load_state_dict(agent.optimizer.state_dict())          # torch's own format: the state moves over as it is
    agent.world = 2                                             # grad_scale 1/2 (nothing is all-reduced here)
    gen = torch.Generator().manual_seed(17)
    scale = 40.0 if clipped else 0.1          # norm of the halved gradient: ~ scale/2 * sqrt(6742) = 1640 or 4.1; max_grad_norm 10
    worst = {}
    for step in range(3):
        grad = torch.randn(n, generator=gen) * scale
        agent.grads.copy_(grad)
        agent._set_hyper()
        with torch.cuda.device(agent.device):
            agent._clip_step(agent._desc)
        torch.cuda.synchronize()
        off = 0
        for p in params:
            p.grad = (grad[off:off + p.numel()] * 0.5).view(p.shape).clone()
            off += p.numel()
        total = torch.nn.utils.clip_grad_norm_(params, cfg.max_grad_norm)
        assert (float(total) > cfg.max_grad_norm) == clipped
        assert (float(agent.scalars[5]) < 1.0) == clipped and abs(float(agent.scalars[3]) - float(total)) < 1e-4 * float(total)
        topt.step()
        pairs = {"parameters": (agent.flat.cpu(), torch.cat([p.detach().reshape(-1) for p in params]))}
        for sname, buf in state_buffers(agent.optimizer).items():
            pairs[sname] = (buf.cpu(), flat_state(topt, params, sname))
        for what, (x, y) in pairs.items():
            worst[what] = max(worst.get(what, 0.0), ulps(x.numpy(), y.numpy()))
            print(f"{name} {'clipped' if clipped else 'unclipped'} step {step} {what}: max abs {float((x - y).abs().max()):.3e}, "
                  f"{ulps(x.numpy(), y.numpy()):.0f} ulp, {int((x != y).sum())} of {n} elements differ")
            np.testing.assert_allclose(x.numpy(), y.numpy(), rtol=0, atol=STEP_TOL, err_msg=f"{what}, step {step}")
    print(f"WORST {name} {'clipped' if clipped else 'unclipped'}: {worst}")
    assert int(agent.optimizer.step_t.item()) == 4          # every kind advances the device counter


# ---------------------------------------------------------------------------------------------- 2. the golden cases
_ORACLE_RUNS = {}


def oracle_run(name):
    """The oracle's trajectory on a fixture (fp32 update with the swapped optimizer + the fp64 gradient of every step),
    evaluated once for both GEMM modes."""
    if name not in _ORACLE_RUNS:
        from oracle.learner_ref import LearnerOracle
        g = H.load_case(name)
        cpu_cfg = H.case_config(g)
        sd, tgt = H.build_init_state(cpu_cfg, int(g["seed"]), C=int(g["C"]), A=int(g["A"]), head_scale=H.case_head_scale(g))
        spec = H.spec_from_config(cpu_cfg, C=int(g["C"]), A=int(g["A"]))
        orc = swap_optimizer(LearnerOracle(sd, spec, tgt), cpu_cfg)
        steps = []
        for step in range(int(g["steps"])):
            batch, w, taus = H.case_batch(g, step)
            rec = dict(g64=orc.grads_fp64(batch, w, taus), pre_sd=orc.state_dict(),
                       pre_tgt=None if orc.p_tgt is None else {k: v.clone() for k, v in orc.p_tgt.items()}, jitter=None)
            rec["td"] = orc.update(batch, w, taus)
            rec["grads"], rec["grad_norm"], rec["post"] = orc.last["grads"], float(orc.last["grad_norm"]), orc.state_dict()
            steps.append(rec)
            if cpu_cfg.use_target_network and step == 0:
                orc.sync_target()
        _ORACLE_RUNS[name] = (cpu_cfg, spec, list(sd.keys()), {k: v.numel() for k, v in sd.items()}, steps)
    return _ORACLE_RUNS[name]


@pytest.mark.parametrize("gemm_mode", ["fp32", "bf16x3"])
@pytest.mark.parametrize("name", NEW_CASES)
def test_update_matches_reference_and_oracle(dev, name, gemm_mode):
    g = H.load_case(name)
    cfg, agent = build_hip_agent(g, dev, gemm_mode=gemm_mode)
    assert not cfg.use_adam
    np.testing.assert_array_equal(np.array([float(v.double().sum()) for v in agent.model.state_dict().values()]), g["init_sum"])
    cpu_cfg, spec, names, numel, steps = oracle_run(name)
    sens = cfg.learning_rate / cfg.rmsprop_epsilon if cfg.use_rmsprop else cfg.learning_rate
    kink_total = 0
    for step, rec in enumerate(steps):
        batch, w, taus = H.case_batch(g, step)
        td = agent.update(to_hip_batch(batch, dev), per_weights=w.to(dev), taus=[t.to(dev) for t in taus])
        torch.cuda.synchronize()
        pre = f"s{step}/"
        np.testing.assert_allclose(td.cpu().numpy(), g[pre + "td"], rtol=0, atol=LOSS_TOL)
        if pre + "dl" in g.files:
            np.testing.assert_allclose(agent._static_distribution_loss.cpu().numpy(), g[pre + "dl"], rtol=0, atol=LOSS_TOL)
        if pre + "ql" in g.files:
            np.testing.assert_allclose(agent._static_q_loss.cpu().numpy(), g[pre + "ql"], rtol=0, atol=LOSS_TOL)
        assert abs(float(agent._static_total_loss) - float(g[pre + "total"])) < LOSS_TOL
        np.testing.assert_allclose(td.cpu().numpy(), rec["td"].numpy(), rtol=0, atol=LOSS_TOL)
        # gradients: tolerance and kink allowance exactly as in tests/test_gpu_learner.py
        off, gflat, kinked, allowance = 0, agent.grads.cpu(), {}, {}
        for k in names:
            n = numel[k]
            go, g64, gh = rec["grads"][k].reshape(-1), rec["g64"][k].reshape(-1), gflat[off:off + n]
            tol = 1e-4 * float(go.abs().max()) + 1e-7
            kink = 2.0 * float((go.double() - g64).abs().max())
            err = min(float((gh - go).abs().max()), float((gh.double() - g64).abs().max()))
            if err > tol + kink:
                if rec["jitter"] is None:
                    rec["jitter"] = H.jitter_grads(rec["pre_sd"], rec["pre_tgt"], spec, batch, w, taus, seed=1234 + step)
                kink = max(kink, 2.0 * max(float((jg[k].reshape(-1) - go).abs().max()) for jg in rec["jitter"]))
            allowance[k] = kink
            if err > tol:
                kinked[k] = err
            assert err <= tol + kink, f"step {step} grad {k}: max err {err:.3e} > {tol:.3e} + {kink:.3e}"
            off += n
        kink_total += len(kinked)
        assert abs(float(agent.scalars[3]) - rec["grad_norm"]) < 1e-4 * max(1.0, rec["grad_norm"])
        post = agent.model.state_dict()
        for k, v in rec["post"].items():
            np.testing.assert_allclose(post[k].cpu().numpy(), v.numpy(), rtol=0, atol=STEP_TOL + sens * allowance[k], err_msg=k)
        l2 = np.array([float(v.double().norm()) for v in post.values()])
        np.testing.assert_allclose(l2, g[pre + "post_l2"], rtol=2e-6, atol=1e-7)
        if cfg.use_target_network and step == 0:
            agent.sync_target_model()
    assert int(agent.optimizer.step_t.item()) == int(g["steps"])
    width = max(cfg.iqn_quantile_model_feature_dim if cfg.use_iqn else 0, cfg.ids_q_head_feature_dim if cfg.use_ids else 0)
    assert kink_total <= 4 and (kink_total == 0 or width >= 256), f"{kink_total} (tensor, step) pairs needed the kink allowance"


# ---------------------------------------------------------------------------------------------- 3. / 6. forms agree
def _mk(dev, fused, graph, B=256, cap=4096, base=2, fuse_tail=True, **over):
    from prism_amd.config import baseline_config
    from prism_amd.learner import Learner
    from prism_amd.synthetic import fill_replay
    knobs = {k: over.pop(k) for k in ("optimizer_entry_points",) if k in over}
    cfg = baseline_config(base, device=dev, batch_size=B, experience_replay_capacity=cap, **over)
    cfg.fused_step, cfg.hip_graph, cfg.fuse_tail = fused, graph, fuse_tail
    for k, v in knobs.items():
        setattr(cfg, k, v)
    ln = Learner()
    with contextlib.redirect_stdout(io.StringIO()):
        ln.configure(cfg, obs_shape=(10, 10, 4), n_actions=6)
    fill_replay(ln.experience_buffer, cap, seed=3)
    return ln


def _snapshot(ln, td):
    buf, ag = ln.experience_buffer, ln.agent
    out = [td.cpu().numpy(), buf._index.cpu().numpy(), buf._weight.cpu().numpy(), ag.flat.cpu().numpy(),
           buf.sum_tree.cpu().numpy(), np.float32(ag.scalars[0].item())]
    return out + [b.cpu().numpy() for b in ag.optimizer.buffers()]


def _run_side_by_side(learners, steps=20):
    for step in range(steps):
        outs = []
        for ln in learners:
            td = ln.step(timesteps_this_iteration=1).clone()
            torch.cuda.synchronize()
            outs.append(_snapshot(ln, td))
        for i, other in enumerate(outs[1:]):
            for j, (x, y) in enumerate(zip(outs[0], other)):
                np.testing.assert_array_equal(x, y, err_msg=f"step {step}, learner {i + 1}, item {j}")
    for ln in learners:
        assert int(ln.agent.optimizer.step_t.item()) == steps
        ln.agent.check_status()


def test_rmsprop_forms_agree_and_repeat(dev):
    """c3 (IQN + PER, B = 256) with RMSprop, 20 steps: sample -> update -> update_priority, the fused launches (post + back),
    their hipGraph replay, and a second fresh hipGraph run, all bit for bit."""
    over = dict(use_adam=False, use_rmsprop=True)
    ref, fus, gra, again = _mk(dev, False, False, **over), _mk(dev, True, False, **over), _mk(dev, True, True, **over), \
        _mk(dev, True, True, **over)
    _run_side_by_side([ref, fus, gra, again])
    assert any(isinstance(g, tuple) for g in gra.agent._graphs.values())          # a graph really was captured
    assert gra.agent._desc.fuse_tail == 0 and type(gra.agent.optimizer).__name__ == "HipRMSprop"
    assert float(gra.agent.optimizer.square_avg.abs().sum()) > 0


def test_adam_through_the_new_entry_points_is_unchanged(dev):
    """Adam over the same 20 steps: prism_learner_clip_adam / prism_step_back against prism_learner_clip_step /
    prism_step_back_opt with PRISM_OPT_ADAM -- graph replay with the fused tail, the post + back pair, the unfused form."""
    new = dict(optimizer_entry_points=True)
    old = _mk(dev, True, True)
    learners = [old, _mk(dev, True, True, **new), _mk(dev, True, True, fuse_tail=False, **new), _mk(dev, False, False, **new)]
    assert not old.agent._opt_calls and all(ln.agent._opt_calls for ln in learners[1:])
    _run_side_by_side(learners)


# ---------------------------------------------------------------------------------------------- 4. checkpoints
def test_reference_rmsprop_checkpoint_loads_and_continues(dev, tmp_path):
    from oracle.learner_ref import LearnerOracle
    g = H.load_case("dqn_c2_rmsprop")
    ck = os.path.join(H.GOLDEN, "ref_checkpoint_rmsprop")
    exp = np.load(os.path.join(H.GOLDEN, "ref_checkpoint_rmsprop_expected.npz"))
    cfg, agent = build_hip_agent(g, dev)
    agent.load(ck)
    s = np.array([float(v.double().sum()) for v in agent.model.state_dict().values()])
    np.testing.assert_array_equal(s, exp["sum"])
    assert int(agent.optimizer.step_t.item()) == 2 and agent.n_updates == int(exp["n_updates"])
    assert abs(float(agent.optimizer.square_avg.double().sum()) - float(exp["square_avg_sum"].sum())) < 1e-9
    assert abs(float(agent.optimizer.grad_avg.double().sum()) - float(exp["grad_avg_sum"].sum())) < 1e-9
    # one further update against the oracle continued from the same files
    cpu_cfg = H.case_config(g)
    model_sd = torch.load(os.path.join(ck, "agent", "model.pt"), map_location="cpu", weights_only=True)
    orc = swap_optimizer(LearnerOracle(model_sd, H.spec_from_config(cpu_cfg, C=4, A=6), None), cpu_cfg)
    orc.opt.load_state_dict(torch.load(os.path.join(ck, "agent", "optimizer.pt"), map_location="cpu", weights_only=True))
    batch, w, taus = H.case_batch(g, 0)
    td_o = orc.update(batch, w, taus)
    td = agent.update(to_hip_batch(batch, dev), per_weights=w.to(dev))
    torch.cuda.synchronize()
    np.testing.assert_allclose(td.cpu().numpy(), td_o.numpy(), rtol=0, atol=LOSS_TOL)
    post, params = agent.model.state_dict(), list(orc.p.values())
    for k, v in orc.state_dict().items():
        np.testing.assert_allclose(post[k].cpu().numpy(), v.numpy(), rtol=0, atol=STEP_TOL, err_msg=k)
    for sname, buf in state_buffers(agent.optimizer).items():
        np.testing.assert_allclose(buf.cpu().numpy(), flat_state(orc.opt, params, sname).numpy(), rtol=0, atol=STEP_TOL, err_msg=sname)
    # save -> load in a fresh agent -> both continue bit-identically
    agent.save(str(tmp_path))
    _, other = build_hip_agent(g, dev)
    other.load(str(tmp_path))
    assert int(other.optimizer.step_t.item()) == 3
    batch, w, taus = H.case_batch(g, 1)
    for a in (agent, other):
        a.update(to_hip_batch(batch, dev), per_weights=w.to(dev))
    torch.cuda.synchronize()
    assert torch.equal(agent.flat, other.flat)
    for x, y in zip(agent.optimizer.buffers(), other.optimizer.buffers()):
        assert torch.equal(x, y)
    # the file a reference Agent.load would read: torch's RMSprop takes it
    sd = torch.load(os.path.join(str(tmp_path), "agent", "optimizer.pt"), map_location="cpu", weights_only=True)
    fresh = [torch.zeros_like(p).requires_grad_(True) for p in params]
    topt = torch.optim.RMSprop(fresh, lr=1.0, centered=True)
    topt.load_state_dict(sd)
    assert float(topt.state[fresh[0]]["step"]) == 3.0 and topt.param_groups[0]["lr"] == cfg.learning_rate


# ---------------------------------------------------------------------------------------------- 5. data parallel
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _dp_worker(rank, world, port, q):
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.cuda.set_device(0)
    from prism_amd import dist as pdist
    from prism_amd.agents import hip_agent
    from prism_amd.config import baseline_config
    from prism_amd.learner import Learner
    from prism_amd.synthetic import fill_replay
    summed = []

    def host_allreduce(flat, group=None):          # gloo over host memory (no RCCL with two ranks on one device)
        h = flat.cpu()
        dist.all_reduce(h)
        flat.copy_(h)
        summed.append(h)
        return 1.0 / world
    hip_agent.pdist.allreduce_grads = host_allreduce

    cfg = baseline_config(2, device="cuda:0", batch_size=32, experience_replay_capacity=2048, use_adam=False, use_rmsprop=True)
    ln = Learner()
    with contextlib.redirect_stdout(io.StringIO()):
        ln.configure(cfg, obs_shape=(10, 10, 4), n_actions=6, process_group=dist.group.WORLD)
    buf, ag = ln.experience_buffer, ln.agent
    assert ag.world == world and type(ag.optimizer).__name__ == "HipRMSprop"
    _, buf.seed, ag.seed = pdist.rank_seeds(cfg.seed, rank)
    fill_replay(buf, 2048, seed=rank)
    idx = []
    for step in range(5):
        ln.step()
        torch.cuda.synchronize()
        assert torch.equal(ag.grads.cpu(), summed[-1])          # what the optimizer kernel read IS the gloo sum
        for t in (ag.flat, ag.optimizer.square_avg, ag.optimizer.grad_avg):
            assert pdist.assert_replicas_identical(t.cpu())
        idx.append(buf._index.cpu().numpy().copy())
    q.put((rank, ag.flat.cpu().numpy(), np.stack(idx), int(ag.optimizer.step_t.item()),
           any(isinstance(g, tuple) and len(g) == 2 for g in ag._graphs.values())))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(600)
def test_two_ranks_with_rmsprop_stay_identical(dev):
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_dp_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = sorted([q.get(timeout=240), q.get(timeout=240)], key=lambda r: r[0])
    for p in procs:
        p.join(60)
        assert p.exitcode == 0
    (_, p0, i0, s0, g0), (_, p1, i1, s1, g1) = res
    np.testing.assert_array_equal(p0, p1)             # replicas bit-identical
    assert not np.array_equal(i0, i1)                 # ... while sampling different transitions
    assert s0 == s1 == 5 and g0 and g1                # the split hipGraph path really ran
