"""CPU: the host restatement of sampled information-directed action selection (tests/select_ref.py) -- the Philox words of
its stream key against common.h compiled for the host, its clamped probabilities against the selector's own torch code on
the acting fixtures, its inverse CDF as a sampler, the counter accounting -- and the argument checks of
``prism_ids_sample_select``.  tests/test_gpu_ids_sampled.py holds the kernel to this restatement draw for draw."""
import subprocess

import numpy as np
import pytest
import torch

from tests import helpers as H
from tests import select_ref as S
from tests.test_philox_host import _HOST_PROGRAM, _hipcc

SEED = 20240917          # the seed of the frequency test, here and on the device
N_DRAWS = 65536


def freq_probs(A):
    """One fixed weight vector per action count: an entry at the clamp floor (1e-10), a dominant one, the rest small and
    unequal; clamped but not normalised, as the kernel samples them."""
    p = np.full(A, 1e-10, dtype=np.float32)
    p[A - 1] = 0.75
    for a in range(1, A - 1):
        p[a] = np.float32(0.2 / (A - 2) * (0.5 + a / (A - 1)))
    return p


def test_ids_key_words_equal_common_h_on_the_host(tmp_path):
    """Philox and u64_to_unit_double of common.h, built for the host alone, at the key "IDSA"."""
    import os
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("no hipcc to compile the host program with")
    src, exe = tmp_path / "ids_key_host.cpp", tmp_path / "ids_key_host"
    src.write_text("#include <string.h>\n" + _HOST_PROGRAM)
    subprocess.run([hipcc, "-x", "hip", "--offload-host-only", "-O1", "-std=c++17", "-ffp-contract=off",
                    "-I", os.path.join(H.ROOT, "include"), "-I", os.path.join(H.ROOT, "prism_amd", "csrc"),
                    str(src), "-o", str(exe)], check=True, capture_output=True, text=True, timeout=300)
    assert S.IDS_KEY == int.from_bytes(b"IDSA", "big") == 0x49445341
    assert S.IDS_KEY not in [H.TAU_KEY + s for s in range(4)] + [0x5045524D, 0x554E4946]
    n = 1024
    for seed, first in ((SEED, 0), (123, 2 ** 32 - 500), (0xFEDCBA9876543210, 2 ** 40 + 11)):
        out = subprocess.run([str(exe), str(seed), str(first), str(S.IDS_KEY), str(n)], check=True, capture_output=True,
                             text=True, timeout=60).stdout.split()
        words = np.array([int(x, 16) for x in out], dtype=np.uint64).reshape(n, 6)
        r = H.philox4x32(seed, np.uint64(first) + np.arange(n, dtype=np.uint64), S.IDS_KEY)
        np.testing.assert_array_equal(words[:, :4].astype(np.uint32), r)
        u = S.ids_uniforms(seed, first, n)
        np.testing.assert_array_equal(words[:, 5].copy().view(np.float64), u)
        assert float(u.min()) >= 0.0 and float(u.max()) < 1.0
    assert S.u64_to_unit_double(np.uint32(0xFFFFFFFF), np.uint32(0xFFFFFFFF)) == 1.0 - 2.0 ** -53


IDS_FIXTURES = [n for n in H.UPDATE_CASES if "act/ids/IDS Scores" in H.load_case(n).files]


@pytest.mark.parametrize("name", IDS_FIXTURES)
def test_clamped_probs_equal_the_selector(name):
    """The selector's own torch code with random_sample set, on the estimates the acting fixtures recorded."""
    from prism_amd.agents import squish_functions
    from prism_amd.agents.action_selectors import IDSActionSelector
    g = H.load_case(name)
    cfg = H.case_config(g)
    _, _, ref = H.case_act(g)
    _, unsquish = squish_functions.parse(cfg.loss_squish_fn_id)
    sel = IDSActionSelector(cfg.ids_lambda, True, cfg.ids_epsilon, cfg.ids_rho_lower_bound, cfg.ids_beta, unsquish)
    probs = sel.generate_action_probs(torch.from_numpy(ref["dist"]), torch.from_numpy(ref["q"]), for_log=True)
    scores = sel.loggables["IDS Scores"].numpy()
    np.testing.assert_allclose(scores, ref["ids/IDS Scores"], rtol=1e-5, atol=0)          # (the reference's recorded scores)
    mine = S.clamped_probs(scores, cfg.ids_epsilon)
    assert mine.dtype == np.float32 and mine.shape == scores.shape
    np.testing.assert_array_equal(mine, probs.numpy())
    assert float(mine.min()) >= np.float32(cfg.ids_epsilon) and float(mine.max()) <= 1.0
    # and on the recorded scores themselves, sign, max subtraction and clamp spelled out in float64
    x = -ref["ids/IDS Scores"].astype(np.float64)
    e = np.exp(x - x.max(axis=1, keepdims=True))
    np.testing.assert_allclose(S.clamped_probs(ref["ids/IDS Scores"], cfg.ids_epsilon),
                               np.clip(e / e.sum(axis=1, keepdims=True), cfg.ids_epsilon, 1.0), rtol=1e-5, atol=0)


def test_inverse_cdf_edges():
    p = np.array([0.25, 0.5, 0.125], dtype=np.float32)
    edges = np.array([0.0, 0.25 / 0.875 - 1e-12, 0.25 / 0.875, 0.75 / 0.875, 1.0 - 2.0 ** -53])
    # t = u * S against cumulative sums 0.25, 0.75, 0.875 (strict "<": a value ON a boundary belongs to the next action)
    t = edges * 0.875
    want = [int(np.searchsorted(np.array([0.25, 0.75, 0.875]), x, side="right")) for x in t]
    np.testing.assert_array_equal(S.inverse_cdf(p, edges), np.minimum(want, 2))
    np.testing.assert_array_equal(S.inverse_cdf(np.array([1e-10], dtype=np.float32), np.array([0.0, 0.999])), [0, 0])
    # rounding brings t up to S: nobody's interval, the last action
    np.testing.assert_array_equal(S.inverse_cdf(p, np.array([1.0])), [2])
    # per-row probabilities
    rows = np.array([[1.0, 1e-10], [1e-10, 1.0]], dtype=np.float32)
    np.testing.assert_array_equal(S.inverse_cdf(rows, np.array([0.5, 0.5])), [0, 1])


@pytest.mark.parametrize("A", [2, 6, 16])
def test_inverse_cdf_is_a_correct_sampler(A):
    """65 536 draws at the seed the GPU test uses: every action's count within 5 standard deviations of N p_a / S."""
    p = freq_probs(A)
    assert np.float32(1e-10) in p and float(p.max()) == 0.75
    act = S.sample_actions(np.broadcast_to(p, (N_DRAWS, A)), SEED, 0)
    assert act.dtype == np.int64 and int(act.min()) >= 0 and int(act.max()) < A
    w = p.astype(np.float64) / p.astype(np.float64).sum()
    counts = np.bincount(act, minlength=A)
    for a in range(A):
        mu, sd = N_DRAWS * w[a], np.sqrt(N_DRAWS * w[a] * (1.0 - w[a]))
        print(f"A={A} action {a}: count {counts[a]}, expected {mu:.2f} +- {sd:.2f}")
        assert abs(counts[a] - mu) <= 5.0 * sd, f"A={A} action {a}: {counts[a]} draws, expected {mu:.2f} +- 5 * {sd:.2f}"


CALL_TABLE = [
    [(4096, 1), (1, 1)],                                   # the widest call first, T = 1: n * T == n, ranges touch
    [(1, 1), (4096, 1), (1, 1), (17, 1)],
    [(1, 200), (17, 200), (1, 200)],
    [(16, 8), (3, 8), (4096, 8), (1, 8)],
    [(5, 1), (5, 200), (4096, 1), (2, 1), (1, 1), (1, 1)],
    [(39, 200), (16, 200), (16, 200), (7, 200)],           # n > cap in pieces: every piece a call of its own
]


@pytest.mark.parametrize("calls", CALL_TABLE)
@pytest.mark.parametrize("c0", [0, 777, 2 ** 32 - 3])
def test_counter_ranges_of_successive_calls_are_disjoint(calls, c0):
    ranges, end = S.call_ranges(c0, calls)
    assert end == c0 + sum(n * T for n, T in calls)
    for (lo0, hi0), (lo1, hi1) in zip(ranges, ranges[1:]):
        assert lo0 < hi0 <= lo1 < hi1, f"counter ranges overlap: [{lo0}, {hi0}) and [{lo1}, {hi1})"
    flat = np.concatenate([np.arange(lo, hi, dtype=np.uint64) for lo, hi in ranges])
    assert len(np.unique(flat)) == len(flat)
    # different counters, different uniforms
    u = np.concatenate([S.ids_uniforms(SEED, lo, hi - lo) for lo, hi in ranges])
    assert len(np.unique(u)) == len(u)


def test_sample_select_argument_checks_without_device():
    import __graft_entry__ as g
    import os
    from prism_amd import _native as N
    if not os.path.exists(N.LIB_PATH):
        g.build()
    L = N.lib()
    p = 4096          # (a non-null address: every check fails before anything is launched or read)

    def call(z=p, q=p, n=4, n_pad=16, T=8, A=6, heads=10, usq=0, scores=p, action=p):
        return L.prism_ids_sample_select(z, q, n, n_pad, T, A, heads, 0.1, 1e-10, 0.25, usq, None, 1, 0, None, scores, None,
                                         None, action, None, None)

    for bad in (dict(z=None), dict(q=None), dict(action=None), dict(scores=None)):
        assert call(**bad) == N.PRISM_ERR_INVALID, bad
        assert b"prism_ids_sample_select: null buffers" in L.prism_last_error()
    for bad in (dict(n=0), dict(n=17), dict(T=0), dict(A=0), dict(A=17), dict(heads=0)):
        assert call(**bad) == N.PRISM_ERR_INVALID, bad
        assert b"prism_ids_sample_select: bad sizes" in L.prism_last_error()
    for bad in (dict(usq=-1), dict(usq=3)):
        assert call(**bad) == N.PRISM_ERR_INVALID, bad
        assert b"unsquish" in L.prism_last_error()
    # the same calls of prism_ids_select answer the same
    assert L.prism_ids_select(p, p, 0, 16, 8, 6, 10, 0.1, 1e-10, 0.25, 0, p, None, p, None, None) == N.PRISM_ERR_INVALID
    assert L.prism_ids_select(p, p, 4, 16, 8, 17, 10, 0.1, 1e-10, 0.25, 0, p, None, p, None, None) == N.PRISM_ERR_INVALID
