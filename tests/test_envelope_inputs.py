"""No GPU needed: what tests/test_gpu_envelope.py rests on, checked on the CPU.

  * the envelope prism_learner_supported accepts, restated in Python and compared over a grid with its neighbours just
    outside; every case of the GPU file lies inside;
  * the launch forms: prism_learner_plan_info (what make_plan decides) equals the `expect` of every case, agrees with a
    Python restatement of the plan's five predicates over a grid with the neighbours of every threshold, and the cases
    reach every form at action counts other than 6 and channel counts other than 4;
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
        B = case.get("B", 32)
        cfg = baseline_config(case["base"], device="cpu", batch_size=B, **case["over"])
        assert lib.prism_learner_supported(ctypes.byref(_dims_of(cfg, case["C"], case["A"])), B) == N.PRISM_OK, name
    # the tables of the issue, row by row: action counts, channels and batch edges the cases reach
    A_seen = {c["A"] for c in E.UPDATE_CASES.values()}
    C_seen = {c["C"] for c in E.UPDATE_CASES.values()}
    B_seen = {c["B"] for c in E.UPDATE_CASES.values()}
    assert {1, 2, 3, 5, 6, 7, 16} <= A_seen and {1, 2, 3, 4, 10} <= C_seen and {1, 2, 3, 4, 5, 17, 4096} <= B_seen


# ------------------------------------------------------------------------------------------------------ launch forms
def _fused_plan(case):
    from prism_amd import _native as N
    from prism_amd.config import baseline_config
    B = case.get("B", 32)
    cfg = baseline_config(case["base"], device="cpu", batch_size=B, **case["over"])
    return N.plan_info(_dims_of(cfg, case["C"], case["A"]), B, str(getattr(cfg, "gemm_mode", "auto")))


def test_every_case_reaches_its_form(lib):
    """prism_learner_plan_info -- what make_plan (prism_amd/csrc/plan.h) decides for the case's dims, batch and mode -- equals
    the `expect` of every update case in every mode it runs, and of every fused-form case in the default mode.  Every case
    names at least the IQN backward, the Q-head backward, who folds the conv backward and the number of gradient slabs."""
    from prism_amd import _native as N
    n = 0
    for name, case in E.UPDATE_CASES.items():
        d = _dims_of(E.case_config(name), case["C"], case["A"])
        for mode in case["modes"]:
            want, got = E.expect_of(case, mode), N.plan_info(d, case["B"], mode)
            assert {"bwd", "q_bwd", "conv_in_bwd", "n_chunks"} <= set(want) <= set(N.PLAN_FIELDS), name
            assert got is not None and {k: got[k] for k in want} == want, (name, mode, want, got)
            assert got["split"] == int(mode == "bf16x3" and got["bwd"] != "none"), (name, mode)
            n += 1
    for name, case in E.FUSED_CASES.items():
        want, got = case["expect"], _fused_plan(case)
        assert got is not None and {k: got[k] for k in want} == want, (name, want, got)
    assert n == sum(len(c["modes"]) for c in E.UPDATE_CASES.values()) > 100


TRUNK_FORMS = [("fp32", 0), ("fp32", 1), ("bw3", 0), ("bw3", 1), ("bw4", 0)]     # (iqn_bwd4_kernel never folds the conv backward in)
Q_FORMS = ["rows", "cols", "qb2"]


def test_every_form_is_reached_away_from_a6_c4(lib):
    """Every (backward of the one-layer IQN trunk, conv_in_bwd) pair and every backward of the two-layer Q heads that the
    predicates of make_plan can produce is reached by update cases at two or more action counts other than 6 and at two or
    more channel counts other than 4.  ("none" and "lin" are picked by the model kind, not by a predicate: rows 4 and 7, and
    tests/iqn_linear_cases.py.)  The fused-form cases reach iqn_bwd3_kernel's 16 slabs at n_params % 4 = 1 and 3 and
    qh_bwd2_kernel with the first Q-head offset at 1 mod 4."""
    from prism_amd import _native as N
    trunk = {f: (set(), set()) for f in TRUNK_FORMS}
    heads = {f: (set(), set()) for f in Q_FORMS}
    for name, case in E.UPDATE_CASES.items():
        d = _dims_of(E.case_config(name), case["C"], case["A"])
        for mode in case["modes"]:
            p = N.plan_info(d, case["B"], mode)
            for table, key in ((trunk, (p["bwd"], p["conv_in_bwd"])), (heads, p["q_bwd"])):
                if key in table:
                    table[key][0].add(case["A"])
                    table[key][1].add(case["C"])
    for key, (As, Cs) in list(trunk.items()) + list(heads.items()):
        assert len(As - {6}) >= 2 and len(Cs - {4}) >= 2, (key, sorted(As), sorted(Cs))
    # the two per-lane channel packings of the folded conv backward, on both sides of T = 8 | T >= 16, and the staging bound
    packed = {(c["C"], E.case_config(n).iqn_n_current_state_quantile_samples) for n, c in E.UPDATE_CASES.items()
              if "bf16x3" in c["modes"] and E.expect_of(c, "bf16x3")["bwd"] == "bw3" and E.expect_of(c, "bf16x3")["conv_in_bwd"]}
    assert packed >= {(2, 8), (4, 8), (8, 16), (4, 64)}
    assert E.UPDATE_CASES["r13_bw3_t16_a3c8_b192"]["expect"]["conv_in_bwd"] == 1
    assert E.UPDATE_CASES["r13_bw3_t16_a3c8_b224"]["expect"]["conv_in_bwd"] == 0
    assert {E.expect_of(c, "bf16x3")["n_chunks"] for c in E.UPDATE_CASES.values()
            if "bf16x3" in c["modes"] and E.expect_of(c, "bf16x3")["bwd"] == "bw4"} == {1, 2, 8}
    bw3 = [c for c in E.FUSED_CASES.values() if c["expect"]["bwd"] == "bw3"]
    assert {c["rem"] for c in bw3} == {1, 3} and all(c["expect"]["n_chunks"] == 16 for c in bw3)
    assert any(c["expect"]["q_bwd"] == "qb2" and c["head_rem"] == 1 for c in bw3)


# The five predicates make_plan asks (bwd3_kernels.h bw3_ok / bw3_conv_ok, bwd4_kernels.h bw4_ok / bw4_chunks, qbwd2_kernels.h
# qb2_ok, and B <= 128 for the Q heads' column form), restated
def bw3_ok(H, B, T):
    return H == 128 and (B * T) % (16 * 32) == 0 and (B * T // 16) % T == 0           # 16 row chunks of whole 32-row blocks, whole samples


def bw3_conv_ok(use_iqn, heads, propagate, T, C, B):
    share = {4: 1, 8: 2}.get(T, 4)               # lanes that hold one (sample, position) value split the channels
    samples = (B * T // 16) // T                 # per row chunk: their observation rows are staged in LDS
    lds = 2 * 3 * 32 * (288 + 160) + 4096 + 4 * (4 * samples * 40 * C + 4 * 4 * 19 + 4 * 96 + 4)
    return bool(use_iqn and heads == 0 and propagate and T >= 8 and C % share == 0 and C // share <= 2
                and (C // share == 1 or C % 2 == 0) and 9 * C < 96 and samples * 10 * C <= 1024 and lds <= 160 * 1024)


def bw4_chunks(B, T):
    R = B * T
    return next((rc for rc in (8, 4, 2, 1) if R % (32 * rc) == 0 and (R // rc) % T == 0), 0)     # (the C list's 16 never wins over 8)


def qb2_ok(H, B, heads, head_layers):
    return H == 128 and head_layers == 2 and B % 128 == 0 and heads >= 2


def plan_forms(C, B, T, use_iqn, heads, head_layers, width, mode, propagate=1):
    """(bwd, conv_in_bwd or None where iqn_bwd_kernel's own rule decides, n_chunks, q_bwd) of make_plan, from the five."""
    heads2 = heads > 0 and head_layers == 2
    split = mode == "bf16x3" and (use_iqn or heads2)
    if use_iqn and split and bw3_ok(width, B, T):
        trunk = ("bw3", int(bw3_conv_ok(use_iqn, heads, propagate, T, C, B)), 16)
    elif use_iqn and split and width == 256 and bw4_chunks(B, T):
        trunk = ("bw4", 0, bw4_chunks(B, T))
    else:
        trunk = ("fp32" if use_iqn else "none", None if use_iqn else 0, 8 if width == 128 or not use_iqn else 4)
    q = "none" if not heads2 else "qb2" if split and qb2_ok(width, B, heads, head_layers) else "cols" if B <= 128 else "rows"
    return trunk + (q,)


PLAN_MODELS = [(True, 0, 0), (True, 10, 2), (True, 2, 2), (True, 1, 2), (True, 16, 2), (False, 10, 2), (False, 1, 2), (False, 1, 1)]
PLAN_BATCHES = (1, 2, 3, 4, 5, 7, 8, 9, 12, 14, 15, 16, 17, 18, 24, 28, 30, 31, 32, 33, 34, 36, 48, 60, 62, 63, 64, 65, 66, 68, 96,
                112, 120, 124, 126, 127, 128, 129, 130, 132, 136, 140, 143, 144, 145, 148, 160, 176, 192, 200, 208, 216, 224, 240,
                248, 252, 254, 255, 256, 257, 258, 260, 264, 272, 384, 512, 640, 1024, 4096)


def test_plan_agrees_with_the_restated_predicates(lib):
    """prism_learner_plan_info against plan_forms over a grid with the neighbours on each side of every threshold: B * T
    around 512 and 1024 for every T (B = 512 / T and 1024 / T with the nearest batches the envelope admits on each side),
    B around 128 and 144, the staging bound's B = 192 | 208 | 224, C = 1 .. 10, T in {4, 8, 16, 32, 64}, both widths, both modes,
    IQN alone / beside 1, 2, 10 and 16 two-layer heads / heads alone / the one-layer DQN head; outside the envelope it
    refuses as prism_learner_supported does."""
    from prism_amd import _native as N
    seen, n_out = {}, 0
    for (use_iqn, heads, hl), width, T, B, mode in itertools.product(PLAN_MODELS, (128, 256), POW2, PLAN_BATCHES, ("fp32", "bf16x3")):
        for C in range(1, 11) if use_iqn and not heads else (1, 4, 8):
            d = make_dims(5, C, T, T, use_iqn, heads, hl, width)
            d.propagate_grad = 1
            got = N.plan_info(d, B, mode)
            if not in_envelope(5, C, B, T, T, use_iqn, heads, hl, width):
                assert got is None, (C, B, T, use_iqn, heads, hl, width, mode)
                n_out += 1
                continue
            bwd, conv, chunks, q = plan_forms(C, B, T, use_iqn, heads, hl, width, mode)
            assert (got["bwd"], got["n_chunks"], got["q_bwd"]) == (bwd, chunks, q), (C, B, T, use_iqn, heads, hl, width, mode, got)
            assert conv is None or got["conv_in_bwd"] == conv, (C, B, T, use_iqn, heads, hl, width, mode, got)
            assert got["q_de_slots"] == (2 if q == "qb2" else heads), (B, heads, hl, width, mode, got)
            key = (got["bwd"], got["conv_in_bwd"], got["n_chunks"], got["q_bwd"])
            seen[key] = seen.get(key, 0) + 1
    assert n_out > 1000 and sum(seen.values()) > 10000
    assert {k[:2] for k in seen} >= set(TRUNK_FORMS) | {("none", 0)} and {k[3] for k in seen} == set(Q_FORMS) | {"none"}
    assert {k[2] for k in seen if k[0] == "bw4"} == {8, 4, 2, 1}
    # without gradient through the embedding (propagate_grad 0) nothing folds the conv backward in; 0 = the default mode, bf16x3
    d = make_dims(5, 4, 8, 8, True, 0, 0, 128)
    assert N.plan_info(d, 64, "bf16x3")["conv_in_bwd"] == 0 and N.plan_info(d, 64, "bf16x3")["bwd"] == "bw3"
    if not os.environ.get("PRISM_GEMM"):
        assert N.plan_info(d, 64, 0) == N.plan_info(d, 64, "bf16x3") != N.plan_info(d, 64, "fp32")


def test_the_thresholds_themselves(lib):
    """The neighbours named one by one (IQN alone, width 128, bf16x3 unless said): what flips, and where."""
    from prism_amd import _native as N

    def plan(B, T=8, C=4, heads=0, width=128, mode="bf16x3"):
        d = make_dims(5, C, T, T, True, heads, 2 if heads else 0, width)
        d.propagate_grad = 1
        p = N.plan_info(d, B, mode)
        return p["bwd"], p["conv_in_bwd"], p["n_chunks"], p["q_bwd"]
    assert plan(62)[0] == "fp32" and plan(64)[:3] == ("bw3", 1, 16) and plan(66)[0] == "fp32" and plan(64, mode="fp32")[0] == "fp32"
    assert plan(126)[0] == "fp32" and plan(128)[0] == "bw3" and plan(130)[0] == "fp32"
    # whole samples per row chunk: 512 rows of T = 64 would give a chunk half a sample, 1536 rows one and a half
    assert plan(16, T=64)[0] == "bw3" and plan(8, T=64)[0] == "fp32" and plan(24, T=64)[0] == "fp32" and plan(32, T=64)[0] == "bw3"
    assert [plan(B, T=16, C=8)[:2] for B in (192, 208, 224)] == [("bw3", 1), ("fp32", 1), ("bw3", 0)]       # (208 * 16 % 512 != 0)
    assert [plan(64, C=C)[1] for C in range(1, 11)] == [0, 1, 0, 1, 0, 0, 0, 0, 0, 0]                      # T = 8: C = 2, 4
    assert [plan(32, T=16, C=C)[1] for C in range(1, 11)] == [0, 0, 0, 1, 0, 0, 0, 1, 0, 0]                # T >= 16: C = 4, 8
    assert [plan(128, T=4, C=C)[1] for C in range(1, 11)] == [0] * 10                                      # T = 4: never
    assert plan(128, heads=10)[3] == "qb2" and plan(112, heads=10)[3] == "cols" and plan(144, heads=10)[3] == "rows"
    assert plan(128, heads=1)[3] == "cols" and plan(128, heads=2)[3] == "qb2" and plan(256, heads=1)[3] == "rows"
    assert plan(128, heads=10, mode="fp32")[3] == "cols" and plan(256, heads=10, mode="fp32")[3] == "rows"
    assert plan(128, heads=10, width=256)[3] == "cols" and plan(128, heads=10)[1] == 0
    assert [plan(B, T=4, width=256)[::2] for B in (4, 8, 16, 32, 64, 128)] == \
        [("fp32", 4), ("bw4", 1), ("bw4", 2), ("bw4", 4), ("bw4", 8), ("bw4", 8)]
    assert plan(4, T=8, width=256)[::2] == ("bw4", 1) and plan(2, T=8, width=256)[0] == "fp32" and plan(12, T=8, width=256)[::2] == ("bw4", 1)


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
