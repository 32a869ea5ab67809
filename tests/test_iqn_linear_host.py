"""No GPU needed: what tests/test_gpu_iqn_linear.py rests on, for the linear IQN head (iqn_quantile_model_layers = 0).

  * the depth-0 rule of prism_learner_supported, restated in Python and compared over a grid: T, T' in {4, 8, 16, 32, 64},
    B*T and B*T' multiples of 16, no Q heads beside it, A 1..16, C 1..10, B 1..4096, and iqn_width does not matter;
    depth 1 keeps the rule of tests/test_envelope_inputs.py and depth 2 stays refused;
  * HipAgent's parameter offsets of depth-0 models, LayerNorm on and off: running sums of named_parameters(), every trunk
    field -1, phi_w a multiple of four floats, phi | [LayerNorm] | head contiguous (the backward's slabs rely on it);
  * prism_learner_workspace_bytes > 0 for them;
  * the two fixtures recorded from the live reference against the oracle, at tests/test_oracle_golden.py's tolerances;
  * the inputs of the fixtures and of every generated case are kink-free by the oracle alone."""
import contextlib
import ctypes
import io
import itertools
import os

import pytest

from tests import helpers as H
from tests import iqn_linear_cases as L
from tests.test_envelope_inputs import in_envelope, make_dims


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from prism_amd import _native as N
    if not os.path.exists(N.LIB_PATH):
        g.build()
    return N.lib()


# ------------------------------------------------------------------------------------------------------ the envelope
POW2 = (4, 8, 16, 32, 64)


def in_envelope_depth(A, C, B, T, Tn, heads, layers, width):
    """IQN models (use_iqn set, `heads` two-layer Q heads of width 128 beside them) by trunk depth."""
    if layers == 1:
        return in_envelope(A, C, B, T, Tn, True, heads, 2 if heads else 0, width)
    if layers != 0:
        return False
    return (heads == 0 and T in POW2 and Tn in POW2 and (B * T) % 16 == 0 and (B * Tn) % 16 == 0 and 1 <= A <= 16
            and 1 <= C <= 10 and 1 <= B <= 4096)


def dims_of(A, C, T, Tn, heads, layers, width):
    d = make_dims(A, C, T, Tn, True, heads, 2 if heads else 0, 128)
    d.iqn_layers, d.iqn_width = layers, width
    return d


def test_depth0_envelope_agrees_with_its_restatement(lib):
    from prism_amd import _native as N
    grid = itertools.product((0, 1, 3, 16, 17), (0, 1, 10, 11), (0, 1, 2, 3, 16, 17, 4096, 4097),
                             ((4, 4), (8, 16), (64, 64), (2, 8), (8, 12)), (0, 1, 10), (0, 1, 2))
    n_in = n_out = 0
    for A, C, B, (T, Tn), heads, layers in grid:
        for width in ((0, 128, 512) if layers == 0 else (128,)):          # the width must not matter without a trunk
            want = in_envelope_depth(A, C, B, T, Tn, heads, layers, width)
            rc = lib.prism_learner_supported(ctypes.byref(dims_of(A, C, T, Tn, heads, layers, width)), B)
            assert rc == (N.PRISM_OK if want else N.PRISM_ERR_UNSUPPORTED), (A, C, B, T, Tn, heads, layers, width, rc)
            n_in, n_out = n_in + int(want and layers == 0), n_out + int(not want)
    assert n_in >= 100 and n_out > 1000


def test_depth0_neighbours(lib):
    from prism_amd import _native as N

    def rc(A=6, C=4, B=32, T=8, Tn=8, heads=0, layers=0, width=128):
        return lib.prism_learner_supported(ctypes.byref(dims_of(A, C, T, Tn, heads, layers, width)), B)
    assert rc() == N.PRISM_OK and rc(width=0) == N.PRISM_OK and rc(width=512) == N.PRISM_OK and rc(B=1, T=16, Tn=16) == N.PRISM_OK
    assert rc(B=4096, T=64, Tn=64, A=16, C=10) == N.PRISM_OK and rc(B=2, T=8, Tn=16) == N.PRISM_OK
    for kw in (dict(layers=2), dict(heads=10), dict(heads=1), dict(B=1), dict(B=3), dict(T=2), dict(Tn=12), dict(A=17), dict(C=11),
               dict(B=4097), dict(layers=1, width=512), dict(layers=1, width=0)):
        assert rc(**kw) == N.PRISM_ERR_UNSUPPORTED, kw
    # the single-Linear DQN head beside a depth-0 IQN: refused like beside a depth-1 one
    d = dims_of(6, 4, 8, 8, 1, 0, 128)
    d.head_layers = 1
    assert lib.prism_learner_supported(ctypes.byref(d), 32) == N.PRISM_ERR_UNSUPPORTED
    for name, case in L.UPDATE_CASES.items():
        from prism_amd.agents.hip_agent import model_dims
        dm = model_dims(L.case_config(name), case["C"], case["A"])
        assert dm.iqn_layers == 0 and lib.prism_learner_supported(ctypes.byref(dm), case["B"]) == N.PRISM_OK, name


# ------------------------------------------------------------------------------------------------------ offsets, workspace
def _model(ln, C, A):
    from prism_amd.factory.model_factory import create_model
    cfg = H.variant_config("cpu", dict(iqn_quantile_model_layers=0, use_layer_norm=ln))
    with contextlib.redirect_stdout(io.StringIO()):
        return cfg, create_model((10, 10, C), A, cfg)


@pytest.mark.parametrize("ln", [True, False])
def test_offsets_of_depth0_models(lib, ln):
    from prism_amd import _native as N
    from prism_amd.agents.hip_agent import _offsets, model_dims
    for C, A in ((4, 6), (1, 1), (10, 16), (3, 3), (2, 2)):
        cfg, m = _model(ln, C, A)
        names = [k for k, _ in m.named_parameters()]
        d = "distribution_model."
        head = [d + "embedding_to_quantile_layer." + s for s in (("0.weight", "0.bias", "1.weight", "1.bias") if ln else ("weight", "bias"))]
        assert names == ["embedding_model.model.0.weight", "embedding_model.model.0.bias", d + "phi.0.weight", d + "phi.0.bias"] + head
        run, table = 0, {}
        for k, p in m.named_parameters():
            table[k] = run
            run += p.numel()
        o = _offsets(m)
        assert o.n_params == run == 16 * (9 * C + 1) + 65 * 1024 + (2048 if ln else 0) + 1024 * A + A and run % 4 == A % 4
        assert (o.conv_w, o.conv_b) == (0, 16 * 9 * C)
        assert o.phi_w == table[d + "phi.0.weight"] == 16 * (9 * C + 1) and o.phi_w % 4 == 0
        assert o.phi_b == table[d + "phi.0.bias"] == o.phi_w + 64 * 1024
        assert (o.iqn_ln1_g, o.iqn_ln1_b, o.iqn_w1, o.iqn_b1) == (-1, -1, -1, -1)
        if ln:
            assert (o.iqn_ln2_g, o.iqn_ln2_b) == (table[head[0]], table[head[1]]) == (o.phi_b + 1024, o.phi_b + 2048)
        else:
            assert (o.iqn_ln2_g, o.iqn_ln2_b) == (-1, -1)
        assert (o.iqn_w2, o.iqn_b2) == (table[head[-2]], table[head[-1]]) == (o.phi_b + 1024 + (2048 if ln else 0), run - A)
        assert o.head_base == -1 and o.h_w1 == -1
        dm = model_dims(cfg, C, A)
        assert dm.iqn_layers == 0
        for B in (16, 2, 256):
            assert lib.prism_learner_supported(ctypes.byref(dm), B) == N.PRISM_OK
            assert lib.prism_learner_workspace_bytes(ctypes.byref(dm), B) > 0


def test_offsets_of_depth1_models_are_unchanged():
    """The rule that tells LayerNorm on from off now looks at the head; models with a trunk map as before."""
    from prism_amd.agents.hip_agent import _offsets
    from prism_amd.factory.model_factory import create_model
    for ln in (True, False):
        cfg = H.variant_config("cpu", dict(use_layer_norm=ln))
        with contextlib.redirect_stdout(io.StringIO()):
            m = create_model((10, 10, 4), 6, cfg)
        table, run = {}, 0
        for k, p in m.named_parameters():
            table[k] = run
            run += p.numel()
        o, d = _offsets(m), "distribution_model."
        i = 1 if ln else 0
        assert o.iqn_w1 == table[d + f"model.model.{i}.weight"] and o.iqn_b1 == table[d + f"model.model.{i}.bias"]
        assert o.iqn_ln1_g == (table[d + "model.model.0.weight"] if ln else -1)
        assert o.iqn_ln2_g == (table[d + "embedding_to_quantile_layer.0.weight"] if ln else -1)
        assert o.iqn_w2 == table[d + ("embedding_to_quantile_layer.1.weight" if ln else "embedding_to_quantile_layer.weight")]
        assert o.iqn_b2 == run - 6


# ------------------------------------------------------------------------------------------------------ fixtures, inputs
@pytest.mark.parametrize("name", L.FIXTURES)
def test_oracle_matches_the_recorded_reference(name):
    from tests.test_oracle_golden import test_oracle_matches_reference_update
    g = H.load_case(name)
    assert H.case_overrides(g)["iqn_quantile_model_layers"] == 0
    test_oracle_matches_reference_update(name)


def _assert_kink_free(label, rows):
    for step, k, gap, move, tol in rows:
        assert gap <= 0.5 * tol, f"{label} step {step} {k}: fp32 / fp64 gap {gap:.3e} > half of {tol:.3e}"
        assert move <= 0.5 * tol, f"{label} step {step} {k}: jitter moves it by {move:.3e} > half of {tol:.3e}"


@pytest.mark.parametrize("name", L.FIXTURES)
def test_fixture_inputs_are_kink_free_by_the_oracle_alone(name):
    cfg, spec, sd, steps = L.fixture_run(name)
    assert len(steps) == 2
    _assert_kink_free(name, [(step,) + row for step, rec in enumerate(steps) for row in L.kink_rows(spec, rec, step)])


@pytest.mark.parametrize("name", list(L.UPDATE_CASES))
def test_generated_inputs_are_kink_free_by_the_oracle_alone(name):
    report = L.kink_report(name)
    assert len({s for s, *_ in report}) == L.UPDATE_CASES[name]["steps"]
    _assert_kink_free(name, report)
    L.forget(name)
