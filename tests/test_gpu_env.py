"""GPU: MinAtar Breakout on the device (``prism_env_breakout_reset`` / ``prism_env_breakout_step``, ``DeviceBreakout``)
against ``HostBreakout`` (tests/env_ref.py), exactly: the case table with given coins and sides, the Philox path, the
ping-pong observation buffers, a captured step, ``VectorCollector`` / ``learn()`` / ``VectorEvaluator`` over the device
environments, and resume.  The runs are tests/game_suite.py's; what is Breakout's own stands here: its learner plays the full
action set through the configuration's own ``build_collector``."""
import numpy as np
import pytest
import torch

from tests import env_cases as EC
from tests import game_suite as GS
from tests.env_frame_cases import GAMES

pytestmark = pytest.mark.gpu
GAME = GAMES["breakout"]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return "cuda:0"


# ---------------------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("obs_dtype", ["float32", "uint8"])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 65])
@pytest.mark.parametrize("group", sorted(EC.GROUPS))
def test_kernel_equals_the_host_restatement_on_the_case_table(dev, group, n, obs_dtype):
    GS.case_table_run(GAME, dev, group, n, obs_dtype)


def test_philox_path_200_steps_at_n_5(dev):
    """The device's own draws (sticky coins, sides, the first side) against the host drawing through philox4x32; the lifetime
    count of environment 1 is about to carry from the first step on."""
    host, (_, terminals, truncations) = GS.philox_run(GAME, dev)
    assert terminals + truncations >= 10 and host.branches["sticky_repeat"] > 100
    assert host.branches["reset_side_0"] and host.branches["reset_side_1"]


def test_the_previous_acting_observation_survives_step(dev):
    GS.ping_pong_check(GAME, dev, lambda k: 3)


def test_a_captured_step_replayed_50_times_equals_an_eager_twin(dev):
    GS.captured_step_run(GAME, dev, obs_dtype="float32")


# ---------------------------------------------------------------------------------------------------- collector, learn, evaluator
def test_vector_collector_rows_equal_a_twin_fed_by_the_host_restatement(dev, tmp_path):
    GS.collector_twin_run(GAME, dev, tmp_path)[2].close()


def test_learn_twice_from_one_seed_is_bit_identical(dev, tmp_path):
    GS.learn_twice_check(GAME, dev, tmp_path, updates=60)


def test_vector_evaluator_over_the_device_equals_eval_host_on_the_restatement(dev):
    from tests.test_gpu_eval import _agent
    GS.evaluator_run(GAME, dev, make_agent=lambda: _agent(dev)[1])


# ---------------------------------------------------------------------------------------------------- resume
def test_state_dict_into_a_fresh_object_continues_bit_identically(dev):
    GS.state_dict_run(GAME, dev, np.random.default_rng(4).integers(0, 3, (60, 6)), other="freeway")


def test_learner_save_state_carries_the_environments_through_the_collector_key(dev, tmp_path):
    GS.save_state_check(GAME, dev, tmp_path)
