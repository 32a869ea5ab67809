"""GPU: ``config.captured_loop`` with ``config.graph_while_filling`` -- ``Learner.learn()`` replaying whole iterations from the
end of the random prologue on, through the fill of the ring, to 20 iterations past it -- against ``learn()`` with both knobs
off from the same seed: bit for bit in everything a run leaves behind (tests/test_gpu_captured_loop.py's comparison and
helpers).  While the ring fills the step's front launch reads the ring's size from the cursor word the LAST of the
iteration's k ingest launches wrote, slot ``p0 ^ (k & 1)``: k = 1 and k = 3 against k = 2 tell that slot from ``p0``.

Shapes: tests/resume_helpers.py (capacity 96, B = 16, N = 5; Seaquest at N = 3), 40 prologue rows."""
import contextlib
import io

import pytest
import torch

from tests import resume_helpers as RH
from tests import test_gpu_captured_loop as CL

pytestmark = pytest.mark.gpu

PAST = 20
NOT_FULL = "the ring is not full yet (its size is baked into the step's launches)"          # the refusal of before
CASES = [(name, tpi) for name in ("iqn_per_egreedy", "ids_sampled", "uniform_target", "freeway_u8") for tpi in (5, 7)] + \
    [("seaquest_n3", 7)]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return "cuda:0"


def _learner(dev, ckpt_dir, name, tpi, limit, captured=True, fill=True, **kw):
    ln, col = CL._learner(dev, ckpt_dir, name, tpi, captured, limit, **kw)
    ln.graph_while_filling = fill
    return ln, col


def _eager(dev, tmp_path_factory, name, tpi, past_fill, **kw):
    return CL._eager_run(dev, tmp_path_factory, name, tpi, past_fill=past_fill, **kw)


@pytest.mark.parametrize("name,tpi", CASES)
def test_both_knobs_on_equal_both_off_across_the_fill(dev, tmp_path, tmp_path_factory, name, tpi):
    n, k, rows0, fill = CL._shape(name, tpi)
    assert k == {5: 1, 7: 2}[tpi] + (name == "seaquest_n3") and fill >= 4
    want = _eager(dev, tmp_path_factory, name, tpi, PAST)
    limit, total = CL._limit(name, tpi, PAST)
    ln, col = _learner(dev, tmp_path, name, tpi, limit)
    got, eager = CL._learn(ln, col)
    assert ln.captured_loop_refusal() is None
    # every update but the two that warm a form up: the cursor form behind the prologue, the by-value form at the fill
    assert ln.captured_iterations == total - 2 and eager == 2 and total == ln.cumulative_model_updates == fill + PAST
    assert got["rows"] == limit and got["size"] == RH.CAPACITY
    RH.assert_same(got, want, f"{name}, {tpi} timesteps per iteration")


@pytest.mark.parametrize("name,tpi", [("iqn_per_egreedy", 5), ("uniform_target", 7), ("seaquest_n3", 7)])
def test_a_run_that_ends_below_capacity(dev, tmp_path, tmp_path_factory, name, tpi):
    want = _eager(dev, tmp_path_factory, name, tpi, -2)
    limit, total = CL._limit(name, tpi, -2)
    ln, col = _learner(dev, tmp_path, name, tpi, limit)
    got, eager = CL._learn(ln, col)
    assert ln.captured_loop_refusal() is None
    assert got["size"] < RH.CAPACITY and total >= 3
    assert ln.captured_iterations == total - 1 and eager == 1          # every update but the one that warmed the form up
    RH.assert_same(got, want, f"{name}, {tpi}: below capacity")


def test_the_fill_knob_switched_off_mid_fill(dev, tmp_path, tmp_path_factory):
    name, tpi = "iqn_per_egreedy", 5
    want = _eager(dev, tmp_path_factory, name, tpi, PAST)
    limit, total = CL._limit(name, tpi, PAST)
    fill = CL._shape(name, tpi)[3]
    half, seen = fill // 2, []
    ln, col = _learner(dev, tmp_path, name, tpi, limit)

    def hook(ln):
        if ln.cumulative_model_updates == half:
            ln.graph_while_filling = False
        if ln.cumulative_model_updates == half + 2:
            seen.append(ln.captured_loop_refusal())
    got, eager = CL._learn(ln, col, hook)
    assert seen == [NOT_FULL]
    # iterations 2 .. half in the cursor form; eager to the fill; one warm-up, then the by-value form
    assert ln.captured_iterations == (half - 1) + (PAST - 1) and eager == total - ln.captured_iterations
    RH.assert_same(got, want, "the fill knob off from mid-fill on")


def test_evaluations_between_replays_mid_fill(dev, tmp_path, tmp_path_factory):
    name, tpi = "iqn_per_egreedy", 5
    limit, total = CL._limit(name, tpi, PAST)
    fill = CL._shape(name, tpi)[3]
    ln, col = _learner(dev, tmp_path, name, tpi, limit, eval_every=20)
    marks = []
    got, eager = CL._learn(ln, col, lambda ln: marks.append((ln.evaluator.evaluations, ln.cumulative_model_updates)))
    assert ln.captured_iterations == total - 2
    assert sum(1 for e, u in marks if 0 < e and u < fill) > 0 and ln.evaluator.evaluations >= 4      # some came mid-fill
    plain, plain_col = _learner(dev, tmp_path / "plain", name, tpi, limit, eval_every=20, evaluate=False)
    want, _ = CL._learn(plain, plain_col)
    assert plain.evaluator is None and plain.captured_iterations == total - 2
    RH.assert_same(got, want, "captured through the fill, with and without evaluations")
    RH.assert_same(want, _eager(dev, tmp_path_factory, name, tpi, PAST, eval_every=20, evaluate=False), "and the eager loop")


def test_resume_mid_fill_in_fresh_objects(dev, tmp_path, tmp_path_factory):
    name, tpi = "iqn_per_egreedy", 7
    (cut, n_cut), (limit, total) = CL._limit(name, tpi, -3), CL._limit(name, tpi, PAST)
    assert n_cut >= 3
    runs = {}
    for knob in (True, False):
        ln, col = _learner(dev, tmp_path / f"first_{knob}", name, tpi, cut, captured=knob, fill=knob, backup_checkpoints=True)
        CL._learn(ln, col)
        assert ln.captured_iterations == (n_cut - 1 if knob else 0)
        runs[knob] = ln.checkpointer.latest_backup()
        assert runs[knob] is not None
    RH.assert_same(CL._parts(runs[True]), CL._parts(runs[False]), "the snapshot taken mid-fill")
    ln, col = _learner(dev, tmp_path / "first_True", name, tpi, cut, backup_checkpoints=True)
    with contextlib.redirect_stdout(io.StringIO()):
        ln.load_state(ln.checkpointer.latest_backup())
    assert ln.experience_buffer._size < RH.CAPACITY
    ln.timestep_limit = limit
    got, eager = CL._learn(ln, col)
    assert ln.captured_iterations == total - n_cut - 2 and eager == 2 and ln.captured_loop_refusal() is None
    want = dict(_eager(dev, tmp_path_factory, name, tpi, PAST))
    # (the device's PER and tau words start at 0 in a fresh agent: tests/test_gpu_captured_loop.py)
    got["rng_counters"], want["rng_counters"] = got["rng_counters"][2:], want["rng_counters"][2:]
    RH.assert_same(got, want, "resumed mid-fill with both knobs on")


def test_without_the_fill_knob_the_refusal_is_the_one_of_before(dev, tmp_path, tmp_path_factory):
    name, tpi = "ids_sampled", 5
    limit, total = CL._limit(name, tpi, -3)
    ln, col = _learner(dev, tmp_path, name, tpi, limit, fill=False)
    got, eager = CL._learn(ln, col)
    assert ln.captured_iterations == 0 and eager == total and ln.captured_loop_refusal() == NOT_FULL
    assert ln.agent.fill_graph_replays == 0
    RH.assert_same(got, _eager(dev, tmp_path_factory, name, tpi, -3), "captured_loop alone, below capacity")


def test_a_serial_behind_the_size_keeps_the_loop_eager_until_full(dev, tmp_path):
    """``_size != min(_serial, capacity)`` (what a load in the reference's format can leave): the cursor word does not hold the
    size, so the loop and the step stay eager until the ring is full, and the refusal says why."""
    name, tpi = "iqn_per_egreedy", 5
    limit, total = CL._limit(name, tpi, PAST)
    fill = CL._shape(name, tpi)[3]
    states, seen = {}, []

    def hook(ln):
        buf = ln.experience_buffer
        if ln.cumulative_model_updates == 0:
            buf._serial += RH.CAPACITY                          # the same slots, another serial: min(serial, capacity) != size
        if ln.cumulative_model_updates == 2 and ln.captured_loop:
            seen.append(ln.captured_loop_refusal())
    for knobs in (True, False):
        ln, col = _learner(dev, tmp_path / str(knobs), name, tpi, limit, captured=knobs, fill=knobs)
        states[knobs], eager = CL._learn(ln, col, hook)
        assert ln.captured_iterations == (PAST - 1 if knobs else 0) and eager + ln.captured_iterations == total == fill + PAST
        assert ln.agent.fill_graph_replays == 0
    assert len(seen) == 1 and "graph_while_filling does not apply" in seen[0] and "write serial is behind its size" in seen[0]
    RH.assert_same(states[True], states[False], "eager until full, captured behind")
