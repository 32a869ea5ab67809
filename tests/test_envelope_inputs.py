"""No GPU needed: what tests/test_gpu_envelope.py rests on, checked on the CPU.

  * the envelope prism_learner_supported accepts, restated in Python and compared over a grid with its neighbours just
    outside; every case of the GPU file lies inside;
  * the alignment facts of the unpadded flat parameter buffer the kernels rely on (phi_w a multiple of 4 floats for every
    A and C) and the remainders the cases are meant to cover (n_params % 4 and the first Q-head offset % 4 over {0, 1, 2, 3});
  * the inputs of every update case are kink-free by the oracle alone: its fp32 and fp64 gradients, and its fp32 gradient
    under a two-ulp parameter jitter, agree within half the gradient tolerance on every tensor of every step -- the check
    tests/test_gpu_variants.py describes in a comment.  The kernels play no part in choosing their own inputs."""
import contextlib
import ctypes
import io
import itertools
import os

import pytest
import torch

from tests import envelope_cases as E
from tests import helpers as H


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from prism_amd import _native as N
    if not os.path.exists(N.LIB_PATH):
        g.build()
    return N.lib()


# ------------------------------------------------------------------------------------------------------ the envelope
POW2 = (4, 8, 16, 32, 64)


def in_envelope(A, C, B, T, Tn, use_iqn, heads, head_layers, width):
    """include/prism_hip.h / README: A 1..16, C 1..10, B 1..4096, width 128 or 256; IQN: T, T' in {4, 8, 16, 32, 64} and
    B*T, B*T' multiples of 16; Q heads: one single-Linear head without IQN, or up to 16 two-layer heads with B % 16 == 0."""
    if not use_iqn and heads == 0:
        return False
    if use_iqn and not (width in (128, 256) and T in POW2 and Tn in POW2 and (B * T) % 16 == 0 and (B * Tn) % 16 == 0):
        return False
    if heads:
        if head_layers == 1:
            if heads != 1 or use_iqn:
                return False
        elif not (head_layers == 2 and 0 < heads <= 16 and width in (128, 256) and B % 16 == 0):
            return False
    return 1 <= B <= 4096 and 1 <= A <= 16 and 1 <= C <= 10


def make_dims(A, C, T, Tn, use_iqn, heads, head_layers, width):
    from prism_amd import _native as N
    d = N.ModelDims()
    d.in_channels, d.n_actions, d.embed_dim, d.use_iqn = C, A, 1024, int(use_iqn)
    d.n_basis, d.iqn_layers, d.iqn_width, d.n_tau, d.n_tau_next, d.use_layer_norm = 64, 1, width, T, Tn, 1
    d.n_heads, d.head_layers, d.head_width = heads, head_layers, width
    return d


MODELS = [(True, 0, 0), (True, 10, 2), (True, 16, 2), (True, 17, 2), (False, 1, 1), (False, 1, 2), (True, 1, 1), (False, 2, 1),
          (False, 0, 0), (True, 10, 3)]          # (use_iqn, heads, head_layers)


def test_supported_envelope_agrees_with_its_restatement(lib):
    from prism_amd import _native as N
    grid = itertools.product((0, 1, 2, 3, 5, 6, 7, 16, 17), (0, 1, 2, 4, 10, 11),
                             (0, 1, 2, 3, 4, 5, 15, 16, 17, 24, 32, 48, 4095, 4096, 4097),
                             ((4, 4), (8, 8), (16, 16), (64, 64), (8, 16), (32, 4), (2, 8), (8, 12), (128, 128)),
                             MODELS, (128, 256, 512))
    n_in = n_out = 0
    for A, C, B, (T, Tn), (use_iqn, heads, hl), width in grid:
        want = in_envelope(A, C, B, T, Tn, use_iqn, heads, hl, width)
        rc = lib.prism_learner_supported(ctypes.byref(make_dims(A, C, T, Tn, use_iqn, heads, hl, width)), B)
        assert rc == (N.PRISM_OK if want else N.PRISM_ERR_UNSUPPORTED), (A, C, B, T, Tn, use_iqn, heads, hl, width, rc)
        n_in, n_out = n_in + int(want), n_out + int(not want)
    assert n_in > 1000 and n_out > 1000


def test_neighbours_just_outside_are_refused(lib):
    from prism_amd import _native as N

    def rc(A=6, C=4, B=32, T=8, Tn=8, use_iqn=True, heads=0, hl=0, width=128):
        return lib.prism_learner_supported(ctypes.byref(make_dims(A, C, T, Tn, use_iqn, heads, hl, width)), B)
    assert rc() == N.PRISM_OK and rc(A=1) == N.PRISM_OK and rc(A=16) == N.PRISM_OK and rc(C=1) == N.PRISM_OK
    assert rc(C=10) == N.PRISM_OK and rc(B=2) == N.PRISM_OK and rc(B=4096) == N.PRISM_OK
    for kw in (dict(A=0), dict(A=17), dict(C=0), dict(C=11), dict(B=0), dict(B=4097), dict(B=1), dict(B=3, T=8, Tn=8),
               dict(B=2, T=4, Tn=4), dict(B=24, heads=10, hl=2), dict(B=24, use_iqn=False, heads=1, hl=2)):
        assert rc(**kw) == N.PRISM_ERR_UNSUPPORTED, kw
    assert rc(B=24) == N.PRISM_OK and rc(B=24, use_iqn=False, heads=1, hl=1) == N.PRISM_OK      # (the rule is the two-layer heads')
    assert rc(B=17, use_iqn=False, heads=1, hl=1) == N.PRISM_OK


def _dims_of(cfg, C, A):
    from prism_amd.agents.hip_agent import model_dims
    return model_dims(cfg, C, A)


def test_every_gpu_case_is_inside_the_envelope(lib):
    from prism_amd import _native as N
    from prism_amd.config import baseline_config
    for name, case in E.UPDATE_CASES.items():
        d = _dims_of(E.case_config(name), case["C"], case["A"])
        assert lib.prism_learner_supported(ctypes.byref(d), case["B"]) == N.PRISM_OK, name
        assert in_envelope(case["A"], case["C"], case["B"], d.n_tau, d.n_tau_next, bool(d.use_iqn), d.n_heads, d.head_layers,
                           d.iqn_width if d.use_iqn else 128), name
    for name, case in E.ACT_CASES.items():
        cfg = H.variant_config("cpu", case["over"])
        assert lib.prism_learner_supported(ctypes.byref(_dims_of(cfg, case["C"], case["A"])), cfg.batch_size) == N.PRISM_OK, name
    for name, case in E.FUSED_CASES.items():
        cfg = baseline_config(case["base"], device="cpu", batch_size=32, **case["over"])
        assert lib.prism_learner_supported(ctypes.byref(_dims_of(cfg, case["C"], case["A"])), 32) == N.PRISM_OK, name
    # the tables of the issue, row by row: action counts, channels and batch edges the cases reach
    A_seen = {c["A"] for c in E.UPDATE_CASES.values()}
    C_seen = {c["C"] for c in E.UPDATE_CASES.values()}
    B_seen = {c["B"] for c in E.UPDATE_CASES.values()}
    assert {1, 2, 3, 5, 6, 7, 16} <= A_seen and {1, 2, 3, 4, 10} <= C_seen and {1, 2, 3, 4, 5, 17, 4096} <= B_seen


# ------------------------------------------------------------------------------------------------------ alignment facts
def _layout(over, C, A):
    cfg = H.variant_config("cpu", over)
    sd, _ = H.build_init_state(cfg, 0, C=C, A=A)
    return E.layout(sd)


def test_phi_w_is_a_multiple_of_four_floats_for_every_A_and_C():
    """The 16-byte reads of the IQN kernels start at phi_w (check_learner refuses anything else): the conv block in front
    of it is 16 * (9 C + 1) floats, whatever A and C are -- a fact, not an accident of the shapes the suite used to run."""
    for over in ({}, E.FULL):
        for C in range(1, 11):
            for A in range(1, 17):
                n, table = _layout(over, C, A)
                phi_w = table["distribution_model.phi.0.weight"]
                assert phi_w == 16 * (9 * C + 1) and phi_w % 4 == 0, (over, C, A)
                assert n % 4 == (A if not over else 11 * A) % 4, (over, C, A)
                if over:
                    assert E.first_head_offset(table) % 4 == A % 4


def test_parameter_counts_and_remainders_of_the_table():
    """n_params, n_params % 4 and the first Q-head offset % 4 (width 128, LayerNorm on) -- the rest of the suite runs the
    A = 6 rows only."""
    rows = [({}, 6, 4, 201_430, 2, None), ({}, 1, 4, 200_785, 1, None), ({}, 5, 4, 201_301, 1, None), ({}, 3, 1, 200_611, 3, None),
            ({}, 7, 3, 201_415, 3, None), ({}, 16, 10, 203_584, 0, None),
            (E.FULL, 6, 4, 1_544_210, 2, 2), (E.FULL, 1, 4, None, 3, 1), (E.FULL, 5, 4, None, 3, 1), (E.FULL, 3, 1, None, 1, 3),
            (E.FULL, 7, 3, None, 1, 3), (E.FULL, 16, 4, None, 0, 0),
            (dict(E.DQN1, use_layer_norm=True), 6, 4, 8_790, 2, 0), (dict(E.DQN1, use_layer_norm=True), 1, 4, None, 1, 0),
            (dict(E.DQN1, use_layer_norm=True), 5, 4, None, 1, 0), (dict(E.DQN1, use_layer_norm=True), 3, 4, None, 3, 0),
            (dict(E.DQN1, use_layer_norm=True), 7, 4, None, 3, 0)]
    for over, A, C, n_want, rem, head_rem in rows:
        n, table = _layout(over, C, A)
        assert n_want is None or n == n_want, (over, A, C, n)
        assert n % 4 == rem, (over, A, C, n)
        head = E.first_head_offset(table)
        assert (None if head is None or head_rem is None else head % 4) == head_rem, (over, A, C, head)


def test_cases_reach_every_remainder():
    """Across the update cases: n_params % 4 and the first Q-head offset % 4 each take all of {0, 1, 2, 3}; the fused-step
    cases are the ones at 1 and 3 (asserted on the device's own buffers in tests/test_gpu_envelope.py)."""
    rems, head_rems = set(), set()
    for name, case in E.UPDATE_CASES.items():
        if case["B"] > 32 or name.startswith(("r6", "r7", "r9")):
            continue
        n, table = _layout(case["over"], case["C"], case["A"])
        rems.add(n % 4)
        head = E.first_head_offset(table)
        if head is not None and name.startswith(("r3", "r5")):
            head_rems.add(head % 4)
    assert rems == {0, 1, 2, 3}
    # (offset 2 is the A = 6 ensemble of tests/test_gpu_learner.py: full_small and the others)
    n, table = _layout(E.FULL, 4, 6)
    assert head_rems | {E.first_head_offset(table) % 4} == {0, 1, 2, 3} and head_rems >= {0, 1, 3}
    assert {c["rem"] for c in E.FUSED_CASES.values()} == {1, 3} and any(c["head_rem"] in (1, 3) for c in E.FUSED_CASES.values())
    for name, case in E.FUSED_CASES.items():
        from prism_amd.config import baseline_config
        from prism_amd.factory.model_factory import create_model
        cfg = baseline_config(case["base"], device="cpu", **case["over"])
        with contextlib.redirect_stdout(io.StringIO()):
            m = create_model((10, 10, case["C"]), case["A"], cfg)
        n, table = E.layout(dict(m.named_parameters()))
        head = E.first_head_offset(table)
        assert n % 4 == case["rem"] and (None if head is None else head % 4) == case["head_rem"], name


# ------------------------------------------------------------------------------------------------------ kink-free inputs
@pytest.mark.parametrize("name", list(E.UPDATE_CASES))
def test_inputs_are_kink_free_by_the_oracle_alone(name):
    """For every (case, step): the oracle's fp32 / fp64 gradient gap and the largest move helpers.jitter_grads produces stay
    under HALF the gradient tolerance on every tensor, i.e. the allowance count of the oracle against itself is zero."""
    report = E.kink_report(name)
    assert len({s for s, *_ in report}) == E.UPDATE_CASES[name]["steps"]
    for step, k, gap, move, tol in report:
        assert gap <= 0.5 * tol, f"{name} step {step} {k}: fp32 / fp64 gap {gap:.3e} > half of {tol:.3e}"
        assert move <= 0.5 * tol, f"{name} step {step} {k}: jitter moves it by {move:.3e} > half of {tol:.3e}"
    E.forget(name)          # (nothing else here needs the trajectory)
