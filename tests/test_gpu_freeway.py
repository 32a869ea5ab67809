"""GPU: MinAtar Freeway on the device (``prism_env_freeway_reset`` / ``prism_env_freeway_step``, ``DeviceFreeway``) against
``HostFreeway`` (tests/freeway_ref.py), exactly: the case table with given coins and speeds, the Philox path, the ping-pong
observation buffers, a captured step, ``VectorCollector`` / ``learn()`` / ``VectorEvaluator`` over the device environments
(C = 7, A = 3; the first 700-byte observation rows to reach ingestion from a device buffer), and resume.  The runs are
tests/game_suite.py's; what is Freeway's own stands here."""
import numpy as np
import pytest
import torch

from tests import freeway_cases as FC
from tests import game_suite as GS
from tests.env_frame_cases import GAMES

pytestmark = pytest.mark.gpu
GAME = GAMES["freeway"]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return "cuda:0"


# ---------------------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("obs_dtype", ["float32", "uint8"])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 65])
@pytest.mark.parametrize("group", sorted(FC.GROUPS))
def test_kernel_equals_the_host_restatement_on_the_case_table(dev, group, n, obs_dtype):
    GS.case_table_run(GAME, dev, group, n, obs_dtype)


def test_philox_path_200_steps_at_n_5(dev):
    """The device's own draws (sticky coins, the first speeds, win and reset speeds) against the host drawing through
    philox4x32.  Hold u: the run must win at least once."""
    host, (wins, _, ends) = GS.philox_run(GAME, dev)
    assert wins >= 1 and ends >= 5 and host.branches["sticky_repeat"] > 100 and host.branches["win"] == wins


def test_given_first_speeds_and_argument_checks(dev):
    env, host = GS.pair(GAME, dev, 3, "uint8")
    first = np.array([FC.SLOW, FC.FAST, FC.SPEEDS], dtype=np.int8)
    np.testing.assert_array_equal(env.reset(first_speeds=first).cpu().numpy().astype(np.float32), host.reset(first_speeds=first))
    GS.assert_env_equal(GAME, env, host, "reset with given speeds")
    np.testing.assert_array_equal(env.get_state()["car_speed"], first)
    with pytest.raises(ValueError, match="8 values per environment"):
        env.reset(first_speeds=first[:2])
    with pytest.raises(ValueError, match="speeds must be"):
        env.step(np.zeros(3, np.int64), speeds=np.zeros((3, 8), np.int8))
    with pytest.raises(ValueError, match="one value per environment"):
        env.step(np.zeros(3, np.int64), u=np.zeros(2))


def test_the_previous_acting_observation_survives_step(dev):
    GS.ping_pong_check(GAME, dev, lambda k: 2)


def test_a_captured_step_replayed_50_times_equals_an_eager_twin(dev):
    rng = np.random.default_rng(8)
    GS.captured_step_run(GAME, dev, acts=np.where(rng.random((51, 9)) < 0.7, 2, rng.integers(0, 6, (51, 9))))


# ---------------------------------------------------------------------------------------------------- collector, learn, evaluator
@pytest.mark.parametrize("obs_storage", ["float32", "uint8"])
def test_vector_collector_rows_equal_a_twin_fed_by_the_host_restatement(dev, tmp_path, obs_storage):
    """Into an fp32 ring and into a byte ring; the device side hands ingestion uint8 observation rows of 700 bytes (4-byte
    aligned only) in the byte case, fp32 rows of 2800 bytes otherwise."""
    ring_d, _, col_d, _ = GS.collector_twin_run(GAME, dev, tmp_path, obs_storage)
    assert ring_d["obs"][:160].reshape(160, -1).float().sum(dim=1).eq(17).all()          # a chicken, eight cars, eight trails a row
    col_d.close()


def test_build_collector_with_the_knob_builds_device_freeway(dev, tmp_path):
    GS.knob_collector_check(GAME, dev, tmp_path).close()


def test_learn_twice_from_one_seed_is_bit_identical(dev, tmp_path):
    GS.learn_twice_check(GAME, dev, tmp_path)


def test_vector_evaluator_over_the_device_equals_eval_host_on_the_restatement(dev):
    GS.evaluator_run(GAME, dev, minimal_actions=True)


# ---------------------------------------------------------------------------------------------------- resume
def test_state_dict_into_a_fresh_object_continues_bit_identically(dev):
    rng = np.random.default_rng(4)
    GS.state_dict_run(GAME, dev, np.where(rng.random((60, 6)) < 0.7, 1, rng.integers(0, 3, (60, 6))), other="breakout")


def test_learner_save_state_carries_the_environments_through_the_collector_key(dev, tmp_path):
    GS.save_state_check(GAME, dev, tmp_path)
