"""GPU: ``graph_while_filling`` on the step alone -- ``HipAgent.step_fused`` replayed from a hipGraph while the ring fills (its
front launch reads the ring's size from the buffer's cursor words), against the twin that launches the step eagerly until the
ring is full.  Every step and everything the run leaves behind, bit for bit.

Shapes: tests/resume_helpers.py (capacity 96, B = 16, N = 5, 40 prologue rows); 30 iterations of 5 rows cross the fill."""
import numpy as np
import pytest
import torch

from tests import resume_helpers as RH

pytestmark = pytest.mark.gpu

PROLOGUE, STEPS = 40, 30
# steps that START below capacity (the step follows the iteration's extend_batch)
BELOW = sum(1 for i in range(STEPS) if PROLOGUE + RH.N_ENV * (i + 1) < RH.CAPACITY)


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return "cuda:0"


def _pair(dev, tmp_path, case):
    """(knob on, knob off): twin learners and scripted collectors from one seed, the random prologue collected.  The knob
    goes where a user puts it: a plain attribute of the configuration, read by ``Learner.configure``."""
    import contextlib
    import io
    from prism_amd.learner import Learner
    out = []
    for knob in (True, False):
        cfg = RH.make_config(case, tmp_path / f"knob_{knob}", dev)
        if knob:
            cfg.graph_while_filling = True
        ln, col = Learner(), RH.ScriptedVectorCollector(seed=3)
        with contextlib.redirect_stdout(io.StringIO()):
            ln.configure(cfg, collector=col)
        assert ln.graph_while_filling is knob
        col.collect_timesteps(PROLOGUE, ln.agent, ln.experience_buffer, random=True)
        ln.cumulative_timesteps = PROLOGUE
        out.append((ln, col))
    return out


def _step_record(ln, col):
    acts, td, scalars = RH.iterate(ln, col)
    buf = ln.experience_buffer
    rec = dict(actions=acts, td=td, scalars=scalars, index=buf._index.cpu().clone())
    if buf.use_per:
        rec["weight"] = buf._weight.cpu().clone()
    return rec


def _graph_steps(agent):
    return [g for g in agent._graphs.values() if isinstance(g, tuple)]


@pytest.mark.parametrize("case", ["a_iqn_per_egreedy_adam", "b_ids_sampled_full", "c_dqn1_uniform_rmsprop"])
def test_the_step_graph_while_filling_equals_the_eager_steps(dev, tmp_path, case):
    assert 2 < BELOW < STEPS - 3
    (on, con), (off, coff) = _pair(dev, tmp_path, case)
    assert on.agent.fill_graph_replays == 0
    for i in range(STEPS):
        RH.assert_same(_step_record(on, con), _step_record(off, coff), f"step {i + 1}")
        below = i < BELOW
        assert on.experience_buffer._size == min(PROLOGUE + RH.N_ENV * (i + 1), RH.CAPACITY)
        if below:
            assert not _graph_steps(off.agent)                  # the twin launches eagerly until the ring is full
            assert bool(_graph_steps(on.agent)) == (i >= 1)
    # every step below capacity but the one that warmed the form up and the one that captured it
    assert on.agent.fill_graph_replays == BELOW - 2 and off.agent.fill_graph_replays == 0
    assert _graph_steps(on.agent) and _graph_steps(off.agent)   # both went over to the by-value graph at the fill
    on.experience_buffer.check_status(), on.agent.check_status()
    RH.assert_same(RH.full_state(on, con), RH.full_state(off, coff), case)


def _stage_rows(ln, rng, n, first_id):
    """``n`` single-row episodes through ``extend()`` (staged on the host until the next flush)."""
    from prism_amd.experience import Timestep
    for j in range(n):
        t = Timestep(id=first_id + j, obs=torch.from_numpy((rng.random_sample((10, 10, RH.C)) < 0.15).astype(np.float32)))
        t.action, t.reward, t.done, t.truncated = int(rng.randint(0, RH.A)), float(rng.standard_normal()), True, False
        ln.experience_buffer.extend(t)


def test_rows_staged_by_extend_between_steps(dev, tmp_path):
    """A row that ``extend()`` stages moves the count on the host alone: the step seeds the cursor word before its replay."""
    (on, con), (off, coff) = _pair(dev, tmp_path, "a_iqn_per_egreedy_adam")
    rngs = np.random.RandomState(5), np.random.RandomState(5)
    taken = 0
    for i in range(7):
        for (ln, _), rng in zip(((on, con), (off, coff)), rngs):
            _stage_rows(ln, rng, 1 + i % 2, 10_000 + 2 * i)
        RH.assert_same(_step_record(on, con), _step_record(off, coff), f"step {i + 1}")
        taken += 1
        assert on.experience_buffer._size < RH.CAPACITY
    assert on.agent.fill_graph_replays == taken - 2
    RH.assert_same(RH.full_state(on, con), RH.full_state(off, coff), "rows staged between steps")


def test_after_a_load_state_mid_fill(dev, tmp_path):
    """A restore moves the count: fresh objects resume mid-fill with the knob on and replay the cursor form again."""
    case = "a_iqn_per_egreedy_adam"
    (on, con), (off, coff) = _pair(dev, tmp_path, case)
    for i in range(4):
        RH.assert_same(_step_record(on, con), _step_record(off, coff), f"step {i + 1}")
    assert on.agent.fill_graph_replays == 2
    on.save_state(tmp_path / "snap")
    new, cnew = RH.make_learner(case, tmp_path / "resumed", dev)
    new.graph_while_filling = True
    new.load_state(tmp_path / "snap")
    assert new.experience_buffer._size == PROLOGUE + 4 * RH.N_ENV == new.experience_buffer._serial
    for i in range(4, STEPS):
        RH.assert_same(_step_record(new, cnew), _step_record(off, coff), f"step {i + 1} (resumed)")
    assert new.agent.fill_graph_replays == BELOW - 4 - 2
    want = RH.full_state(off, coff)
    got = RH.full_state(new, cnew)
    RH.assert_same(got, want, "resumed mid-fill")
