"""GPU: MinAtar Space Invaders on the device (``prism_env_invaders_reset`` / ``prism_env_invaders_step``,
``DeviceSpaceInvaders``) against ``HostSpaceInvaders`` (tests/invaders_ref.py: full 10 x 10 maps moved with ``np.roll``),
exactly: the case table with given coins, the Philox path, the ping-pong observation buffers, a captured step,
``VectorCollector`` / ``learn()`` / ``VectorEvaluator`` over the device environments (C = 6, A = 4), and resume.  The runs are
tests/game_suite.py's; what is this game's own stands here.  Neither side is checked against the ``minatar`` package."""
import numpy as np
import pytest
import torch

from tests import game_suite as GS
from tests import invaders_cases as IC
from tests.env_frame_cases import GAMES

pytestmark = pytest.mark.gpu
GAME = GAMES["invaders"]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return "cuda:0"


# ---------------------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("obs_dtype", ["float32", "uint8"])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 65])
@pytest.mark.parametrize("group", sorted(IC.GROUPS))
def test_kernel_equals_the_host_restatement_on_the_case_table(dev, group, n, obs_dtype):
    GS.case_table_run(GAME, dev, group, n, obs_dtype)


def test_philox_path_300_steps_at_n_5(dev):
    """The device's own sticky coins against the host drawing through philox4x32."""
    host, (kills, terminals, truncations) = GS.philox_run(GAME, dev)
    assert kills >= 1 and terminals >= 1 and truncations >= 1 and host.branches["turn_at_column_0"] + host.branches["turn_at_column_9"] >= 1
    assert host.branches["sticky_repeat"] > 100 and host.branches["alien_shot"] >= 1 and host.branches["fire"] >= 1


def test_given_coin_argument_checks(dev):
    env, host = GS.pair(GAME, dev, 3, "uint8", sticky_action_prob=0.5)
    np.testing.assert_array_equal(env.reset().cpu().numpy().astype(np.float32), host.reset())
    acts = torch.full((3,), 5, dtype=torch.int64, device=dev)
    with pytest.raises(ValueError, match="one value per environment"):
        env.step(acts, u=np.zeros(2))
    with pytest.raises(TypeError):
        env.step(acts, None, np.zeros((3, 3), np.uint8))          # no draw array: the game draws only the coin
    GS.assert_env_equal(GAME, env, host, "after the refusals")          # none of them stepped
    u = np.array([0.1, 0.5, 0.9])
    for k in range(4):
        GS.assert_step_equal(env.step(acts, u=u), host.step(np.full(3, 5), u=u), f"step {k}")
    GS.assert_env_equal(GAME, env, host, "given coins")
    assert list(env.get_state()["last_action"]) == [0, 5, 5]
    env.close()


def test_the_previous_acting_observation_survives_step(dev):
    GS.ping_pong_check(GAME, dev, lambda k: 1 + 2 * (k % 3))


def test_a_captured_step_replayed_50_times_equals_an_eager_twin(dev):
    eager, want = GS.captured_step_run(GAME, dev)
    assert sum(float(w[1].sum()) for w in want) >= 1


# ---------------------------------------------------------------------------------------------------- collector, learn, evaluator
@pytest.mark.parametrize("obs_storage", ["float32", "uint8"])
def test_vector_collector_rows_equal_a_twin_fed_by_the_host_restatement(dev, tmp_path, obs_storage):
    ring_d, _, col_d, _ = GS.collector_twin_run(GAME, dev, tmp_path, obs_storage)
    set_elements = ring_d["obs"][:160].reshape(160, -1).float().sum(dim=1)
    assert set_elements.ge(3).all() and set_elements.le(52).all() and set_elements.max() >= 49          # the cannon and the full block
    assert len(ring_d["action"][:160].unique()) > 2 and int(ring_d["action"][:160].max()) == 3
    col_d.close()


def test_build_collector_with_the_knob_builds_device_space_invaders(dev, tmp_path):
    GS.knob_collector_check(GAME, dev, tmp_path).close()


def test_learn_twice_from_one_seed_is_bit_identical(dev, tmp_path):
    GS.learn_twice_check(GAME, dev, tmp_path)


def test_vector_evaluator_over_the_device_equals_eval_host_on_the_restatement(dev):
    GS.evaluator_run(GAME, dev, minimal_actions=True)


# ---------------------------------------------------------------------------------------------------- resume
def test_state_dict_into_a_fresh_object_continues_bit_identically(dev):
    GS.state_dict_run(GAME, dev, np.random.default_rng(4).integers(0, 4, (60, 6)), other="breakout")


def test_learner_save_state_carries_the_environments_through_the_collector_key(dev, tmp_path):
    GS.save_state_check(GAME, dev, tmp_path)
