"""CPU: the host restatement of epsilon-greedy selection per observation (tests/egreedy_ref.py) -- its stream key and counter
accounting, its anneal against the selector's own ``LinearAnneal``, its coins and random actions as samplers -- the
argument checks of ``prism_egreedy_select`` and what the ``e_greedy_per_env`` knob leaves alone while it is off.
tests/test_gpu_egreedy.py holds the kernel and the agent to this restatement draw for draw."""
import dataclasses
import math

import numpy as np
import pytest

from tests import egreedy_ref as R
from tests import helpers as H
from tests import select_ref as S

SEED = 123
N_DRAWS = 2 ** 18


def test_stream_key_and_counter_ranges():
    assert R.EGREEDY_KEY == int.from_bytes(b"EGRD", "big") == 0x45475244
    others = [H.TAU_KEY + s for s in range(4)] + [0x5045524D, 0x554E4946, S.IDS_KEY]          # TAU0 + sid, PERM, UNIF, IDSA
    assert R.EGREEDY_KEY not in others and len(set(others)) == len(others)
    for s0 in (0, 777, 2 ** 32 - 3):
        for calls in ([1, 1, 1], [4096, 1, 17], [5, 39, 16, 7, 1], [3, 64, 17, 1, 1, 2]):
            ranges, end = R.call_ranges(s0, calls)
            assert end == s0 + sum(calls)
            assert ranges[0][0] == s0 and all(hi - lo == n for (lo, hi), n in zip(ranges, calls))
            for (lo0, hi0), (lo1, hi1) in zip(ranges, ranges[1:]):
                assert lo0 < hi0 == lo1 < hi1, "successive calls: contiguous, disjoint"
            # a call in pieces draws what the call in one piece draws; different counters, different coins
            whole = R.draws(SEED, s0, 0, sum(calls), 6)
            parts = [R.draws(SEED, lo, 0, hi - lo, 6) for lo, hi in ranges]
            rows = [R.draws(SEED, s0, lo - s0, hi - lo, 6) for lo, hi in ranges]
            for k in (0, 1):
                np.testing.assert_array_equal(np.concatenate([p[k] for p in parts]), whole[k])
                np.testing.assert_array_equal(np.concatenate([p[k] for p in rows]), whole[k])
            assert len(np.unique(whole[0])) == len(whole[0])
    # the stream is the key's own: the same counters under "IDSA" give other uniforms
    assert not np.array_equal(R.draws(SEED, 0, 0, 64, 6)[0], S.ids_uniforms(SEED, 0, 64))


@pytest.mark.parametrize("start,stop,max_steps", [(1.0, 0.1, 100_000), (1.0, 0.01, 1000), (0.9, 0.05, 997), (1, 0, 640),
                                                  (0.3, 0.3, 500), (1.0, 0.1, 0), (0.25, 0.75, 333)])
def test_anneal_is_bit_equal_to_linear_anneal(start, stop, max_steps):
    """A walk of uneven call sizes across ``max_steps`` (and beyond): the restated value after every call equals the
    class's ``update(n)``, bit for bit."""
    from prism_amd.agents.action_selectors import LinearAnneal
    a = LinearAnneal(start, stop, max_steps)
    rng = np.random.default_rng(max_steps)
    step, crossed = 0, False
    limit = max(3 * max_steps // 2, 200)
    assert R.anneal(start, stop, max_steps, 0) == a.get_value()
    while step < limit:
        n = int(rng.choice([1, 1, 3, 5, 16, 17, 64, max(1, max_steps // 7)]))
        got = a.update(n)
        step += n
        want = R.anneal(start, stop, max_steps, step)
        assert a.current_step == step
        assert np.float64(got).tobytes() == np.float64(want).tobytes(), f"step {step}: {got!r} != {want!r}"
        assert min(start, stop) - 1e-15 <= want <= max(start, stop) + 1e-15          # (a rounding of the two products apart)
        crossed |= step >= max_steps
    assert crossed and R.anneal(start, stop, max_steps, step) == stop
    if max_steps == 0:
        assert all(R.anneal(start, stop, max_steps, s) == stop for s in (0, 1, 2 ** 40))
    elif start == stop:          # (in between the sum of the two products may round one place off: still the class's bits)
        assert all(R.anneal(start, stop, max_steps, s) == stop for s in (0, max_steps, max_steps + 1))
    else:
        assert R.anneal(start, stop, max_steps, 0) == start
        assert R.anneal(start, stop, max_steps, max_steps - 1) != stop


def test_frequencies_on_the_host():
    """2^18 rows at eps = 0.25 from seed 123: the explore count within 5 sigma of N eps (1109 of 65536), every one of the
    A = 6 random-action counts among the exploring rows within 5 sigma of its binomial mean."""
    A, eps = 6, 0.25
    greedy = np.full(N_DRAWS, -1, dtype=np.int64)          # (no action: marks the rows that did not explore)
    act, explored, got_eps = R.select(greedy, SEED, 0, 0, N_DRAWS, A, eps, eps, 0)
    assert got_eps == eps and explored.dtype == np.uint8
    count = int(explored.sum())
    sd = math.sqrt(N_DRAWS * eps * (1 - eps))
    print(f"explored {count} of {N_DRAWS}, expected {N_DRAWS * eps:.0f} +- {sd:.1f}")
    assert abs(sd - 221.7) < 0.05 and 5 * sd < 1109
    assert abs(count - N_DRAWS * eps) <= 5 * sd
    assert ((act == -1) == (explored == 0)).all()
    picks = act[explored == 1]
    assert int(picks.min()) == 0 and int(picks.max()) == A - 1
    counts = np.bincount(picks, minlength=A)
    for a in range(A):
        mu, sd_a = count / A, math.sqrt(count * (1 / A) * (1 - 1 / A))
        print(f"action {a}: {counts[a]} of {count}, expected {mu:.1f} +- {sd_a:.1f}")
        assert abs(counts[a] - mu) <= 5 * sd_a
    # eps = 1 always explores, eps = 0 never
    assert R.select(greedy[:4096], SEED, 0, 0, 4096, A, 1.0, 1.0, 0)[1].all()
    assert not R.select(greedy[:4096], SEED, 0, 0, 4096, A, 0.0, 0.0, 0)[1].any()
    assert R.select(greedy[:8], SEED, 0, 0, 8, A, 1.0, 1.0, 0, coins=np.full(8, 1.0 - 2.0 ** -53))[1].all()
    assert not R.select(greedy[:8], SEED, 0, 0, 8, A, 0.0, 0.0, 0, coins=np.zeros(8))[1].any()


def _lib():
    import os
    import __graft_entry__ as g
    from prism_amd import _native as N
    if not os.path.exists(N.LIB_PATH):
        g.build()
    return N, N.lib()


def test_egreedy_argument_checks_without_device():
    N, L = _lib()
    p = 4096          # (a non-null address: every check fails before anything is launched or read)

    def call(z=p, q=p, n=4, n_pad=16, T=8, A=6, heads=10, start=1.0, stop=0.1, steps=1000, row0=0, n_call=4, word=None,
             action=p):
        return L.prism_egreedy_select(z, q, n, n_pad, T, A, heads, start, stop, steps, 1, 0, row0, n_call, word, None, None, None,
                                      None, action, None, None)

    refusals = [
        (dict(action=None), b"out_action is null"),
        (dict(z=None, q=None), b"z and q are both null"),
        (dict(n=0, n_call=0), b"bad sizes"), (dict(n=-1), b"bad sizes"), (dict(n=17, n_call=17), b"bad sizes"),
        (dict(A=0), b"bad sizes"), (dict(A=17), b"bad sizes"), (dict(A=-3), b"bad sizes"),
        (dict(heads=0), b"bad sizes"), (dict(z=None, heads=-1), b"bad sizes"),
        (dict(q=None, T=0), b"bad sizes"), (dict(q=None, T=-8), b"bad sizes"),
        (dict(steps=-1), b"anneal_steps is negative"),
        (dict(start=-0.01), b"epsilon outside [0, 1]"), (dict(start=1.5), b"epsilon outside [0, 1]"),
        (dict(stop=-1e-9), b"epsilon outside [0, 1]"), (dict(stop=1.0000001), b"epsilon outside [0, 1]"),
        (dict(start=float("nan")), b"epsilon outside [0, 1]"), (dict(stop=float("nan")), b"epsilon outside [0, 1]"),
        (dict(start=float("inf")), b"epsilon outside [0, 1]"), (dict(stop=float("-inf")), b"epsilon outside [0, 1]"),
        (dict(row0=-1), b"rows outside the call"), (dict(row0=1), b"rows outside the call"),
        (dict(n_call=3), b"rows outside the call"), (dict(row0=2 ** 31 - 2, n_call=2 ** 31 - 1), b"rows outside the call"),
        (dict(word=p, row0=4, n_call=8), b"steps_word needs the whole call"),
        (dict(word=p, n_call=5), b"steps_word needs the whole call"),
    ]
    for bad, text in refusals:
        assert call(**bad) == N.PRISM_ERR_INVALID, bad
        msg = L.prism_last_error()
        assert msg.startswith(b"prism_egreedy_select: ") and text in msg, (bad, msg)
    assert "prism_egreedy_select" in N.SIGNATURES and "prism_egreedy_select(" in open(N.HEADER_PATH).read()
    assert L.prism_abi_version() == 3


def test_knob_off_leaves_factory_presets_and_config_alone(monkeypatch):
    import prism_amd.config as config
    from prism_amd.agents import action_selectors
    from prism_amd.factory import agent_factory
    assert "e_greedy_per_env" in config.__doc__
    assert "e_greedy_per_env" not in {f.name for f in dataclasses.fields(config.Config)}
    presets = [config.DEFAULT_CONFIG, config.MINATAR_CONFIG, config.ADDITIVE_ABLATION_BASE_CONFIG,
               config.SUBTRACTIVE_ABLATION_BASE_CONFIG] + [config.baseline_config(i) for i in range(5)]
    assert not any(hasattr(c, "e_greedy_per_env") for c in presets)
    assert [c.use_e_greedy for c in presets] == [False, False, True, False, True, True, False, False, False]
    built = []

    class Recorder:
        def __init__(self, model, selector, eval_selector, target_model, cfg, in_channels, n_actions, process_group=None):
            built.append((selector, eval_selector))

    monkeypatch.setattr(agent_factory, "HipAgent", Recorder)
    for knob in (None, False, True):          # the knob never changes WHAT is built: the selector stays the reference's class
        cfg = config.baseline_config(0, device="cpu")
        if knob is not None:
            cfg.e_greedy_per_env = knob
        agent_factory.build_agent(cfg, (10, 10, 4), 6)
        sel, ev = built[-1]
        assert type(sel) is action_selectors.EGreedyActionSelector and type(ev) is action_selectors.GreedyActionSelector
        assert (sel.epsilon.start, sel.epsilon.stop, sel.epsilon.max_steps, sel.epsilon.current_step) == (1.0, 0.1, 100_000, 0)
        assert sel.rng.get_state()[1][0] == np.random.RandomState(cfg.seed).get_state()[1][0]
