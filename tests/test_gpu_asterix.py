"""GPU: MinAtar Asterix on the device (``prism_env_asterix_reset`` / ``prism_env_asterix_step``, ``DeviceAsterix``) against
``HostAsterix`` (tests/asterix_ref.py), exactly: the case table with given coins and spawns, the Philox path, the ping-pong
observation buffers, a captured step, ``VectorCollector`` / ``learn()`` / ``VectorEvaluator`` over the device environments
(C = 4, A = 5: the first five-action minimal set), and resume.  The runs are tests/game_suite.py's; what is Asterix's own
stands here.  Neither side is checked against the ``minatar`` package."""
import numpy as np
import pytest
import torch

from tests import asterix_cases as AC
from tests import game_suite as GS
from tests.env_frame_cases import GAMES

pytestmark = pytest.mark.gpu
GAME = GAMES["asterix"]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return "cuda:0"


# ---------------------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("obs_dtype", ["float32", "uint8"])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 65])
@pytest.mark.parametrize("group", sorted(AC.GROUPS))
def test_kernel_equals_the_host_restatement_on_the_case_table(dev, group, n, obs_dtype):
    GS.case_table_run(GAME, dev, group, n, obs_dtype)


def test_philox_path_300_steps_at_n_5(dev):
    """The device's own draws (sticky coins, spawns) against the host drawing through philox4x32."""
    host, (golds, terminals, truncations) = GS.philox_run(GAME, dev)
    assert golds >= 1 and terminals >= 1 and truncations >= 1 and host.branches["exit_left"] + host.branches["exit_right"] >= 1
    assert host.branches["sticky_repeat"] > 100 and host.branches["spawn_gold"] >= 1 and host.branches["spawn_enemy"] >= 1


def test_given_spawn_argument_checks(dev):
    env, host = GS.pair(GAME, dev, 3, "uint8")
    np.testing.assert_array_equal(env.reset().cpu().numpy().astype(np.float32), host.reset())
    GS.assert_env_equal(GAME, env, host, "reset")
    acts = torch.zeros(3, dtype=torch.int64, device=dev)
    with pytest.raises(ValueError, match="3 values per environment"):
        env.step(acts, spawn=np.zeros((2, 3), np.uint8))
    for bad in ([2, 0, 0], [0, 2, 0], [0, 0, 8]):
        with pytest.raises(ValueError, match="spawn must be"):
            env.step(acts, spawn=np.array([[0, 0, 0], bad, [1, 1, 7]]))
    with pytest.raises(ValueError, match="one value per environment"):
        env.step(acts, u=np.zeros(2))
    GS.assert_env_equal(GAME, env, host, "after the refusals")          # none of them stepped
    spawn = np.array([[1, 1, 7], [0, 0, 0], [1, 0, 3]], np.uint8)
    for k in range(12):          # the first spawn falls in here, from the given triples
        GS.assert_step_equal(env.step(acts, spawn=spawn), host.step(acts, spawn=spawn), f"step {k}")
    GS.assert_env_equal(GAME, env, host, "given spawns")
    assert list(env.get_state()["ent_active"].sum(axis=1)) == [1, 1, 1] and list(env.get_state()["ent_active"][:, [7, 0, 3]].diagonal()) == [1, 1, 1]
    env.close()


def test_the_previous_acting_observation_survives_step(dev):
    GS.ping_pong_check(GAME, dev, lambda k: 1 + k % 4)


def test_a_captured_step_replayed_50_times_equals_an_eager_twin(dev):
    eager, want = GS.captured_step_run(GAME, dev)
    assert int(eager.get_state()["ent_active"].sum()) >= 1


# ---------------------------------------------------------------------------------------------------- collector, learn, evaluator
@pytest.mark.parametrize("obs_storage", ["float32", "uint8"])
def test_vector_collector_rows_equal_a_twin_fed_by_the_host_restatement(dev, tmp_path, obs_storage):
    ring_d, _, col_d, _ = GS.collector_twin_run(GAME, dev, tmp_path, obs_storage)
    set_elements = ring_d["obs"][:160].reshape(160, -1).float().sum(dim=1)
    assert set_elements.ge(1).all() and set_elements.le(17).all() and set_elements.max() >= 3          # the player, and entities with trails
    assert len(ring_d["action"][:160].unique()) > 2 and int(ring_d["action"][:160].max()) == 4
    col_d.close()


def test_build_collector_with_the_knob_builds_device_asterix(dev, tmp_path):
    GS.knob_collector_check(GAME, dev, tmp_path).close()


def test_learn_twice_from_one_seed_is_bit_identical(dev, tmp_path):
    GS.learn_twice_check(GAME, dev, tmp_path)


def test_vector_evaluator_over_the_device_equals_eval_host_on_the_restatement(dev):
    GS.evaluator_run(GAME, dev, minimal_actions=True)


# ---------------------------------------------------------------------------------------------------- resume
def test_state_dict_into_a_fresh_object_continues_bit_identically(dev):
    GS.state_dict_run(GAME, dev, np.random.default_rng(4).integers(0, 5, (60, 6)), other="breakout")


def test_learner_save_state_carries_the_environments_through_the_collector_key(dev, tmp_path):
    GS.save_state_check(GAME, dev, tmp_path)
