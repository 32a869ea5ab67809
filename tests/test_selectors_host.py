"""CPU: the MinRegret and SimpleIDS action selectors (prism/agents/action_selectors.py:85-111, :195-286) away from the
device -- the host restatement of the two kernels (tests/select_ens_ref.py) and the two product classes against the
reference's recorded outputs (tests/golden/selectors_ref.npz, written by tools/gen_selector_golden.py from the seeded
table tests/selector_cases.py), the argument checks of ``prism_min_regret_select`` / ``prism_simple_ids_select``, the two
factory knobs and the ``state.pkl`` interchange.  tests/test_gpu_selectors.py holds the kernels and the agent to the same
fixture.

Tolerances (tests/selector_cases.py ``TOL``): rtol 2e-4 / atol 1e-7 without an unsquish function, rtol 1e-3 / atol 1e-6 with
one -- what tests/test_gpu_acting.py holds the IDS scores to.  Actions are compared exactly: the table's seeds were walked
until no row was near a tie in the reference's own scores, by five times these tolerances.  The torch classes' VALUES are
compared with the unsquish function evaluated in float64 (``unsquish_fn``): torch's fp32 sqrt is not the same on every CPU,
and the generator kept only cases whose recorded values that form reproduces within half the tolerance; their actions
are compared with the function as it is, too."""
import dataclasses
import os

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import select_ens_ref as E
from tests import selector_cases as T

FIX = np.load(os.path.join(H.GOLDEN, "selectors_ref.npz"))


def recorded(prefix=""):
    return {k: FIX[prefix + k] for k in ("mr_action", "mr_scores", "mr_spread", "si_action", "si_scaled", "si_mean", "si_max_diff")}


def table_items():
    """(case, q, the case's slice of the fixture: dict of [2][n] actions, [2][n, A] scores, [n, A] values)."""
    f = recorded()
    for c, (r0, r1, v0, v1) in zip(T.cases(), T.layout()):
        shape = (c["n"], c["A"])
        yield c, T.case_q(c), {k: (v[..., r0:r1] if k.endswith("action") else v[..., v0:v1].reshape(v.shape[:-1] + shape))
                               for k, v in f.items()}


def golden_items():
    for name in T.GOLDEN_CASES:
        g = H.load_case(name)
        usq = str(H.case_overrides(g).get("loss_squish_fn_id", "none"))
        q = np.ascontiguousarray(g["act/q"], dtype=np.float32)
        n, A, heads = q.shape
        f = recorded(f"g/{name}/")
        yield (dict(index=name, n=n, A=A, heads=heads, unsquish=usq if usq in T.UNSQUISH else "none"), q,
               {k: (v if k.endswith("action") else v.reshape(v.shape[:-1] + (n, A))) for k, v in f.items()})


def close(got, want, unsquish, what):
    rtol, atol = T.tol(unsquish)
    np.testing.assert_allclose(got, want, rtol=rtol, atol=atol, err_msg=str(what))


def unsquish_fn(name, exact=False):
    """The selector's unsquish function.  ``exact``: evaluated in float64 and rounded to fp32 once -- the same on every
    CPU, where torch's fp32 sqrt and exp differ by an ulp from one CPU to the next (seen: the last elements of a [17, 2]
    tensor), which obs_look_further's (root - 1) turns into 3e-6 relative and a centred mean near zero into more than any
    relative tolerance.  The generator kept only cases whose recorded values lie within half the tolerance of this form."""
    from prism_amd.agents import squish_functions as Q
    fn = {"none": None, "symlog": Q.symexp, "obs_look_further": Q.obs_look_further_squish_fn_inverse}[name]
    return (lambda x: fn(x.double()).float()) if exact and fn is not None else fn


def test_fixture_is_whole_and_free_of_near_ties():
    """From the fixture alone: every row of every table case is there, at both lambdas and both betas, and none is near a
    tie; the recorded golden cases keep all their rows (theirs may be near one: at most one row each is)."""
    rows, values = sum(c["n"] for c in T.cases()), sum(c["n"] * c["A"] for c in T.cases())
    assert len(T.cases()) == 36 and T.layout()[-1][1] == rows and T.layout()[-1][3] == values
    assert {c["n"] for c in T.cases()} == set(T.NS) and {c["unsquish"] for c in T.cases()} == set(T.UNSQUISH)
    for axis, vals in (("A", T.AS), ("heads", T.HEADS), ("unsquish", T.UNSQUISH)):
        assert {(c["n"], c[axis]) for c in T.cases()} == {(n, v) for n in T.NS for v in vals}, axis
    f = recorded()
    assert f["mr_action"].shape == f["si_action"].shape == (2, rows)
    assert f["mr_scores"].shape == f["si_scaled"].shape == (2, values)
    assert f["mr_spread"].shape == f["si_mean"].shape == f["si_max_diff"].shape == (values,)
    assert all(np.isfinite(v).all() for v in f.values())
    assert os.path.getsize(os.path.join(H.GOLDEN, "selectors_ref.npz")) <= 100_000
    for c, q, r in table_items():
        for i in (0, 1):
            assert not T.near_ties(r["mr_scores"][i], c["unsquish"], largest=False).any(), c
            assert not T.near_ties(r["si_scaled"][i], c["unsquish"], largest=True).any(), c
            np.testing.assert_array_equal(r["mr_action"][i], r["mr_scores"][i].argmin(-1))
            np.testing.assert_array_equal(r["si_action"][i], r["si_scaled"][i].argmax(-1))
    for c, q, r in golden_items():
        assert r["mr_action"].shape == r["si_action"].shape == (2, c["n"]) and c["heads"] == 10
        near = sum(int(T.near_ties(r["mr_scores"][i], c["unsquish"], False).sum()) +
                   int(T.near_ties(r["si_scaled"][i], c["unsquish"], True).sum()) for i in (0, 1))
        assert near <= 1, c


def kept(scores, unsquish, largest):
    return ~T.near_ties(scores, unsquish, largest)


@pytest.mark.parametrize("items", [table_items, golden_items])
def test_host_restatement_reproduces_the_reference(items):
    n_rows = 0
    for c, q, r in items():
        usq = c["unsquish"]
        for i, lm in enumerate(T.LAMBDAS):
            got = E.min_regret(q, lm, usq)
            k = kept(r["mr_scores"][i], usq, False)
            np.testing.assert_array_equal(got["action"][k], r["mr_action"][i][k], err_msg=str((c, lm)))
            close(got["scores"], r["mr_scores"][i], usq, (c, lm, "regret^2"))
            close(got["spread"], r["mr_spread"], usq, (c, "spread"))
            close(got["mean"], r["si_mean"], usq, (c, "mean"))          # (the same ensemble mean; MinRegret keeps none)
            n_rows += int(k.sum())
        for i, beta in enumerate(T.BETAS):
            got = E.simple_ids(q, beta, usq)
            k = kept(r["si_scaled"][i], usq, True)
            np.testing.assert_array_equal(got["action"][k], r["si_action"][i][k], err_msg=str((c, beta)))
            close(got["scores"], r["si_scaled"][i], usq, (c, beta, "scaled"))
            close(got["mean"], r["si_mean"], usq, (c, "mean"))
            close(got["max_diff"], r["si_max_diff"], usq, (c, "max_diff"))
            if usq == "none":          # the reference sums the heads one after the other too: the same bits
                np.testing.assert_array_equal(got["mean"], r["si_mean"])
                np.testing.assert_array_equal(got["max_diff"], r["si_max_diff"])
    assert n_rows >= (2 * 504 if items is table_items else 2 * 14)


@pytest.mark.parametrize("items", [table_items, golden_items])
def test_product_classes_reproduce_the_reference(items):
    from prism_amd.agents import action_selectors as S

    class Log:
        def __init__(self):
            self.seen = {}

        def log_data(self, data, group_name, var_name):
            self.seen[(group_name, var_name)] = data

    for c, q, r in items():
        usq, t = c["unsquish"], torch.from_numpy(q)
        dist = torch.zeros((1, c["n"], c["A"]))
        for i, lm in enumerate(T.LAMBDAS):
            sel = S.MinRegretActionSelector(lm, unsquish_fn(usq))
            before = t.clone()
            act = sel.select_action(sel.generate_action_probs(dist, t))
            assert act.dtype == torch.int64 and tuple(act.shape) == (c["n"],) and torch.equal(t, before)
            k = kept(r["mr_scores"][i], usq, False)
            np.testing.assert_array_equal(act.numpy()[k], r["mr_action"][i][k], err_msg=str((c, lm)))
            pinned = S.MinRegretActionSelector(lm, unsquish_fn(usq, exact=True))
            np.testing.assert_array_equal(pinned.select_action(pinned.generate_action_probs(dist, t)).numpy()[k],
                                          r["mr_action"][i][k], err_msg=str((c, lm)))
            close(pinned.regret_squared(t).numpy(), r["mr_scores"][i], usq, (c, lm))
        for i, beta in enumerate(T.BETAS):
            sel = S.SimpleIDSActionSelector(0.1, False, 1e-10, 0.25, beta, unsquish_fn(usq))
            heads = [t[:, :, h].clone() for h in range(c["heads"])]
            keep = [h.clone() for h in heads]
            p_list = sel.generate_action_probs(dist, heads, for_log=True)
            assert all(torch.equal(a, b) for a, b in zip(heads, keep)), "the per-head list was written to"
            lg = {k_: v.numpy() for k_, v in sel.loggables.items()}
            p_tensor = sel.generate_action_probs(dist, t, for_log=True)
            assert torch.equal(p_list, p_tensor) and torch.equal(t, before)
            for k_, v in sel.loggables.items():
                np.testing.assert_array_equal(v.numpy(), lg[k_], err_msg=f"tensor layout != list layout: {k_}")
            assert sorted(lg) == ["Action Probs", "Action Uncertainty", "Q Estimate Ensemble Mean", "Q Estimate Max Difference",
                                  "Scaled Q Values"]
            act = sel.select_action(p_list)
            k = kept(r["si_scaled"][i], usq, True)
            np.testing.assert_array_equal(act.numpy()[k], r["si_action"][i][k], err_msg=str((c, beta)))
            np.testing.assert_array_equal(lg["Action Uncertainty"], lg["Q Estimate Max Difference"])
            np.testing.assert_array_equal(lg["Action Probs"], np.eye(c["A"], dtype=np.int64)[act.numpy()])
            # the values: with the unsquish function pinned (unsquish_fn), so that they are the same on every CPU
            pinned = S.SimpleIDSActionSelector(0.1, False, 1e-10, 0.25, beta, unsquish_fn(usq, exact=True))
            act = pinned.select_action(pinned.generate_action_probs(dist, t, for_log=True))
            np.testing.assert_array_equal(act.numpy()[k], r["si_action"][i][k], err_msg=str((c, beta)))
            lg = {k_: v.numpy() for k_, v in pinned.loggables.items()}
            close(lg["Scaled Q Values"], r["si_scaled"][i], usq, (c, beta))
            close(lg["Q Estimate Ensemble Mean"], r["si_mean"], usq, c)
            close(lg["Q Estimate Max Difference"], r["si_max_diff"], usq, c)
            log = Log()
            pinned.log(log, dist, t)
            assert sorted(log.seen) == [("Debug/SimpleIDS", k_) for k_ in sorted(lg)]
            assert log.seen[("Debug/SimpleIDS", "Scaled Q Values")] == [[round(x, 4) for x in row]
                                                                         for row in lg["Scaled Q Values"].tolist()]


def test_product_classes_refuse_what_the_reference_gets_wrong():
    from prism_amd.agents import action_selectors as S
    with pytest.raises(ValueError, match="two heads"):          # (NaN scores and action 0 in the reference)
        S.MinRegretActionSelector(0.1).generate_action_probs(None, torch.zeros((3, 6, 1)))
    sampled = S.SimpleIDSActionSelector(0.1, True, 1e-10, 0.25, 0.8)
    with pytest.raises(ValueError, match="no sampled form"):          # (RuntimeError out of torch.multinomial there)
        sampled.select_action(sampled.generate_action_probs(None, torch.zeros((3, 6, 2))))
    # the reference's instance attribute names: state.pkl pickles these objects
    assert set(vars(S.MinRegretActionSelector(0.1))) == {"logger", "loggables", "lmbda", "unsquish_function"}
    assert set(vars(sampled)) == set(vars(S.IDSActionSelector(0.1, True, 1e-10, 0.25, 0.8)))
    assert isinstance(sampled.softmax, torch.nn.Softmax)


def _lib():
    import __graft_entry__ as g
    from prism_amd import _native as N
    if not os.path.exists(N.LIB_PATH):
        g.build()
    return N, N.lib()


def test_argument_checks_without_device():
    N, L = _lib()
    p = 4096          # (a non-null address: every check fails before anything is launched or read)
    nan = float("nan")

    def mr(q=p, n=4, n_pad=16, A=6, heads=10, lmbda=0.1, usq=0, action=p):
        return L.prism_min_regret_select(q, n, n_pad, A, heads, lmbda, usq, None, None, action, None, None)

    def si(q=p, n=4, n_pad=16, A=6, heads=10, beta=0.8, usq=0, action=p):
        return L.prism_simple_ids_select(q, n, n_pad, A, heads, beta, usq, None, None, action, None, None)

    shared = [(dict(q=None), b"null buffers"), (dict(action=None), b"null buffers"),
              (dict(n=0), b"bad sizes"), (dict(n=-1), b"bad sizes"), (dict(n=17), b"bad sizes"), (dict(n_pad=3), b"bad sizes"),
              (dict(A=0), b"bad sizes"), (dict(A=17), b"bad sizes"), (dict(A=-3), b"bad sizes"),
              (dict(heads=17), b"n_heads"), (dict(heads=0), b"n_heads"), (dict(heads=-2), b"n_heads"),
              (dict(usq=-1), b"unknown unsquish function"), (dict(usq=3), b"unknown unsquish function")]
    for call, name, extra in ((mr, b"prism_min_regret_select", [(dict(heads=1), b"n_heads"), (dict(lmbda=nan), b"lmbda is NaN")]),
                              (si, b"prism_simple_ids_select", [(dict(beta=nan), b"beta is NaN")])):
        for bad, text in shared + extra:
            assert call(**bad) == N.PRISM_ERR_INVALID, (name, bad)
            msg = L.prism_last_error()
            assert msg.startswith(name + b": ") and text in msg, (bad, msg)
        assert name.decode() in N.SIGNATURES and name.decode() + "(" in open(N.HEADER_PATH).read()
    assert L.prism_abi_version() == 3


def test_accepted_call_reaches_the_launch():
    """One accepted call of each entry point: past every check (one head is fine for SimpleIDS, infinite scalars are no
    NaN).  Without a device the launch itself fails, with PRISM_ERR_HIP and never PRISM_ERR_INVALID; with one it runs on
    real buffers."""
    N, L = _lib()
    if torch.cuda.is_available():
        q = torch.zeros((2, 16, 6), device="cuda")
        act = torch.empty(4, dtype=torch.int64, device="cuda")
        assert L.prism_min_regret_select(N.ptr(q), 4, 16, 6, 2, float("inf"), 2, None, None, N.ptr(act), None, None) == N.PRISM_OK
        assert L.prism_simple_ids_select(N.ptr(q), 4, 16, 6, 1, float("-inf"), 1, None, None, N.ptr(act), None, None) == N.PRISM_OK
        torch.cuda.synchronize()
        return
    p = 4096
    rc = L.prism_min_regret_select(p, 4, 16, 6, 2, float("inf"), 2, None, None, p, None, None)
    assert rc == N.PRISM_ERR_HIP and b"launch failed" in L.prism_last_error()
    rc = L.prism_simple_ids_select(p, 4, 16, 6, 1, float("-inf"), 1, None, None, p, None, None)
    assert rc == N.PRISM_ERR_HIP and b"launch failed" in L.prism_last_error()


def _recorder(monkeypatch):
    from prism_amd.factory import agent_factory
    built = []

    class Recorder:
        def __init__(self, model, selector, eval_selector, target_model, cfg, in_channels, n_actions, process_group=None):
            built.append((selector, eval_selector))

    monkeypatch.setattr(agent_factory, "HipAgent", Recorder)
    return agent_factory, built


def test_factory_knobs(monkeypatch):
    import prism_amd.config as config
    from prism_amd.agents import action_selectors as S, squish_functions as Q
    agent_factory, built = _recorder(monkeypatch)
    for knob in ("ids_action_selector", "eval_action_selector"):
        assert knob in config.__doc__ and knob not in {f.name for f in dataclasses.fields(config.Config)}
    presets = [config.DEFAULT_CONFIG, config.MINATAR_CONFIG, config.ADDITIVE_ABLATION_BASE_CONFIG,
               config.SUBTRACTIVE_ABLATION_BASE_CONFIG] + [config.baseline_config(i) for i in range(5)]
    assert not any(hasattr(c, "ids_action_selector") or hasattr(c, "eval_action_selector") for c in presets)
    ids_attrs = ("lmbda", "random_sample", "epsilon", "ids_rho_lower_bound", "beta", "unsquish_function")

    def build(**over):
        knobs = {k: over.pop(k) for k in ("ids_action_selector", "eval_action_selector") if k in over}
        cfg = config.derive(config.MINATAR_CONFIG, device="cpu", **over)
        for k, v in knobs.items():
            setattr(cfg, k, v)
        agent_factory.build_agent(cfg, (10, 10, 4), 6)
        return cfg, built[-1]

    # knobs absent, or at their defaults: exactly today's selectors and constructor arguments
    for knobs in ({}, dict(ids_action_selector="ids", eval_action_selector="greedy")):
        for squish, fn in (("none", None), ("symlog", Q.symexp), ("obs_look_further", Q.obs_look_further_squish_fn_inverse)):
            cfg, (sel, ev) = build(loss_squish_fn_id=squish, **knobs)
            assert cfg.use_ids and type(sel) is S.IDSActionSelector and type(ev) is S.GreedyActionSelector
            assert [getattr(sel, a) for a in ids_attrs] == [cfg.ids_lambda, cfg.ids_use_random_samples, cfg.ids_epsilon,
                                                            cfg.ids_rho_lower_bound, cfg.ids_beta, fn]
        cfg, (sel, ev) = build(use_ids=False, use_e_greedy=True, **knobs)
        assert type(sel) is S.EGreedyActionSelector and type(ev) is S.GreedyActionSelector
        cfg, (sel, ev) = build(use_ids=False, use_e_greedy=False, **knobs)
        assert type(sel) is S.GreedyActionSelector and type(ev) is S.GreedyActionSelector
    # each knob builds its object
    cfg, (sel, ev) = build(ids_action_selector="simple_ids", loss_squish_fn_id="symlog")
    assert type(sel) is S.SimpleIDSActionSelector and type(ev) is S.GreedyActionSelector and cfg.ids_beta == 0.8
    assert [getattr(sel, a) for a in ids_attrs] == [cfg.ids_lambda, False, cfg.ids_epsilon, cfg.ids_rho_lower_bound, 0.8, Q.symexp]
    cfg, (sel, ev) = build(eval_action_selector="min_regret", loss_squish_fn_id="obs_look_further")
    assert type(sel) is S.IDSActionSelector and type(ev) is S.MinRegretActionSelector
    assert (ev.lmbda, ev.unsquish_function) == (cfg.ids_lambda, Q.obs_look_further_squish_fn_inverse)
    cfg, (sel, ev) = build(ids_action_selector="simple_ids", eval_action_selector="min_regret")
    assert type(sel) is S.SimpleIDSActionSelector and type(ev) is S.MinRegretActionSelector and ev.unsquish_function is None


def test_factory_refusals_come_before_any_model(monkeypatch):
    import prism_amd.config as config
    from prism_amd.factory import model_factory
    agent_factory, built = _recorder(monkeypatch)

    def no_model(*a, **k):
        raise AssertionError("a model was built before the knobs were checked")

    monkeypatch.setattr(model_factory, "create_model", no_model)
    refused = [
        (dict(), dict(ids_action_selector="simple"), "ids_action_selector must be"),
        (dict(), dict(eval_action_selector="minregret"), "eval_action_selector must be"),
        (dict(), dict(eval_action_selector=None), "eval_action_selector must be"),
        (dict(use_ids=False), dict(ids_action_selector="simple_ids"), "need use_ids"),
        (dict(use_ids=False, use_e_greedy=True), dict(eval_action_selector="min_regret"), "need use_ids"),
        (dict(ids_use_random_samples=True), dict(ids_action_selector="simple_ids"), "no sampled form"),
    ]
    for over, knobs, text in refused:
        cfg = config.derive(config.MINATAR_CONFIG, device="cpu", **over)
        for k, v in knobs.items():
            setattr(cfg, k, v)
        with pytest.raises(ValueError, match=text):
            agent_factory.build_agent(cfg, (10, 10, 4), 6)
    assert not built


def test_ref_pickle_both_directions():
    from prism_amd.agents import action_selectors as S, squish_functions as Q
    from prism_amd.util import ref_pickle
    # the reference-written file comes to life as the local classes, with the reference's attributes
    with open(os.path.join(H.GOLDEN, "ref_state_min_regret", "state.pkl"), "rb") as f:
        raw = f.read()
    assert b"prism.agents.action_selectors" in raw and b"MinRegretActionSelector" in raw and b"prism_amd" not in raw
    st = ref_pickle.loads(raw)
    ev, sel = st["eval_action_selector"], st["action_selector"]
    assert type(ev) is S.MinRegretActionSelector and type(sel) is S.SimpleIDSActionSelector
    assert (ev.lmbda, ev.unsquish_function) == (0.1, None)
    assert (sel.lmbda, sel.random_sample, sel.epsilon, sel.ids_rho_lower_bound, sel.beta) == (0.1, False, 1e-10, 0.25, 0.8)
    assert st["n_updates"] == 2 and st["max_grad_norm"] == 10.0 and st["use_cuda_graph"] is False
    assert set(vars(ev)) == set(vars(S.MinRegretActionSelector(0.1)))
    assert set(vars(sel)) == set(vars(S.SimpleIDSActionSelector(0.1, False, 1e-10, 0.25, 0.8)))
    c, q, r = next(table_items())
    t = torch.from_numpy(q)
    np.testing.assert_array_equal(ev.select_action(ev.generate_action_probs(None, t)).numpy(), r["mr_action"][0])
    np.testing.assert_array_equal(sel.select_action(sel.generate_action_probs(None, t)).numpy(), r["si_action"][0])
    # written here, the file names the reference's module for both; a dump followed by a load is a round trip
    state = {"action_selector": S.SimpleIDSActionSelector(0.1, False, 1e-10, 0.25, 0.5, Q.symexp), "n_updates": 3,
             "eval_action_selector": S.MinRegretActionSelector(1.0, Q.obs_look_further_squish_fn_inverse),
             "max_grad_norm": 10.0, "use_cuda_graph": False}
    data = ref_pickle.dumps(state)
    assert b"prism_amd" not in data
    for name in (b"MinRegretActionSelector", b"SimpleIDSActionSelector"):
        assert b"cprism.agents.action_selectors\n" + name + b"\n" in data
    back = ref_pickle.loads(data)
    assert type(back["eval_action_selector"]) is S.MinRegretActionSelector
    assert type(back["action_selector"]) is S.SimpleIDSActionSelector
    for key in ("action_selector", "eval_action_selector"):
        a, b = vars(state[key]), vars(back[key])
        assert set(a) == set(b)
        assert all(a[k] == b[k] for k in a if k != "softmax"), key
    assert back["eval_action_selector"].unsquish_function is Q.obs_look_further_squish_fn_inverse
    assert back["action_selector"].unsquish_function is Q.symexp and back["n_updates"] == 3
    assert ref_pickle.dumps(back) == data
