"""GPU: MinAtar Seaquest on the device (``prism_env_seaquest_reset`` / ``prism_env_seaquest_step``, ``DeviceSeaquest``) against
``HostSeaquest`` (tests/seaquest_ref.py: five Python lists per environment), exactly: the case table with given coins and
spawns, the Philox path, the ping-pong observation buffers, a captured step, ``VectorCollector`` / ``learn()`` /
``VectorEvaluator`` over the device environments (C = 10, A = 6), resume, and the overflow bit.  The runs are
tests/game_suite.py's; what is Seaquest's own stands here.  Neither side is checked against the ``minatar`` package."""
import numpy as np
import pytest
import torch

from tests import game_suite as GS
from tests import resume_helpers as RH
from tests import seaquest_cases as SC
from tests.env_frame_cases import GAMES

pytestmark = pytest.mark.gpu
GAME = GAMES["seaquest"]


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return "cuda:0"


# ---------------------------------------------------------------------------------------------------- the kernel
@pytest.mark.parametrize("obs_dtype", ["float32", "uint8"])
@pytest.mark.parametrize("n", [1, 3, 4, 5, 65])
@pytest.mark.parametrize("group", sorted(SC.GROUPS))
def test_kernel_equals_the_host_restatement_on_the_case_table(dev, group, n, obs_dtype):
    """The cases of the overflow group drop the same append on both sides and raise the status bit."""
    GS.case_table_run(GAME, dev, group, n, obs_dtype)


def test_the_overflow_bit_is_sticky_and_check_status_clears_it(dev):
    from prism_amd import _native as N
    n = 3
    env, host = GS.pair(GAME, dev, n)
    state, actions, u, draws = SC.vector("overflow", n)
    env.set_state(state)
    host.set_state(state)
    env.step(actions[0], u=u[0], draws=draws[0])
    host.step(actions[0], u=u[0], draws=draws[0])
    assert int(env._status.item()) == N.ENV_STATUS_OVERFLOW and host.overflow
    for k in range(3):          # further steps overflow nothing; the bit stays
        env.step(np.zeros(n, np.int64), u=np.ones(n), draws=np.tile(SC.DRAWS, (n, 1)))
        host.step(np.zeros(n, np.int64), u=np.ones(n), draws=np.tile(SC.DRAWS, (n, 1)))
    assert int(env._status.item()) == N.ENV_STATUS_OVERFLOW
    GS.assert_env_equal(GAME, env, host, "after the overflow")          # the append was dropped on both sides, nothing else
    with pytest.raises(N.PrismError, match="DeviceSeaquest: a step appended to a full entity list"):
        env.check_status()
    env.check_status()          # cleared
    env.step(np.full(n, 9), u=np.ones(n), draws=np.tile(SC.DRAWS, (n, 1)))
    with pytest.raises(N.PrismError, match=r"outside \[0, 6\)"):
        env.close()


def test_philox_path_300_steps_at_n_5(dev):
    """The device's own coins and spawn draws against the host drawing through philox4x32."""
    host, (_, terminals, truncations) = GS.philox_run(GAME, dev)
    br = host.branches
    assert terminals >= 1 and truncations >= 1 and br["spawn_fish"] >= 1 and br["spawn_sub"] >= 1 and br["spawn_diver"] >= 1
    assert br["sticky_repeat"] > 100 and br["fire"] >= 1 and not host.overflow


def test_philox_path_at_the_hardest_ramp(dev):
    """Long lists: 200 steps from the hardest ramp (a spawn every step, enemies that move every third), the device's own draws."""
    n = 4
    env, host = GS.pair(GAME, dev, n, sticky_action_prob=0.1)
    host.reset()
    st = host.get_state()
    st["e_spawn_speed"][:], st["move_speed"][:], st["ramp_index"][:], st["e_spawn_timer"][:] = 1, 2, 19, 0
    st["sub_x"][:], st["sub_y"][:], st["surface"][:] = [1, 3, 6, 8], [2, 4, 6, 8], 0
    env.set_state(st)
    host.set_state(st)
    rng = np.random.default_rng(3)
    longest = 0
    for k in range(200):
        acts = rng.integers(0, 6, n)
        GS.assert_step_equal(env.step(acts), host.step(acts), f"step {k}")
        GS.assert_env_equal(GAME, env, host, f"step {k}")
        longest = max([longest] + [len(e["e_fish"]) + len(e["e_subs"]) for e in host.envs])
        if any(e["ep_steps"] == 0 for e in host.envs):          # an episode that ended begins at the hardest ramp again
            st = host.get_state()
            fresh = st["ep_steps"] == 0
            st["e_spawn_speed"][fresh], st["move_speed"][fresh], st["ramp_index"][fresh], st["e_spawn_timer"][fresh] = 1, 2, 19, 0
            env.set_state(st)
            host.set_state(st)
    assert longest >= 8 and host.branches["sub_fires"] >= 3 and not host.overflow
    env.close()


def test_given_draw_argument_checks(dev):
    env, host = GS.pair(GAME, dev, 3, "uint8", sticky_action_prob=0.5)
    np.testing.assert_array_equal(env.reset().cpu().numpy().astype(np.float32), host.reset())
    acts = torch.full((3,), 5, dtype=torch.int64, device=dev)
    with pytest.raises(ValueError, match="one value per environment"):
        env.step(acts, u=np.zeros(2))
    with pytest.raises(ValueError, match="5 values per environment"):
        env.step(acts, None, np.ones((3, 3), np.uint8))
    with pytest.raises(ValueError, match="draws must be"):
        env.step(acts, None, np.zeros((3, 5), np.uint8))
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
    GS.captured_step_run(GAME, dev)


# ---------------------------------------------------------------------------------------------------- collector, learn, evaluator
@pytest.mark.parametrize("obs_storage", ["float32", "uint8"])
def test_vector_collector_rows_equal_a_twin_fed_by_the_host_restatement(dev, tmp_path, obs_storage):
    ring_d, _, col_d, _ = GS.collector_twin_run(GAME, dev, tmp_path, obs_storage)
    set_elements = ring_d["obs"][:160].reshape(160, -1).float().sum(dim=1)
    assert set_elements.ge(2).all() and set_elements.max() >= 12          # the sub and its rear cell; a reset's image has 12
    assert len(ring_d["action"][:160].unique()) > 2 and int(ring_d["action"][:160].max()) == 5
    col_d.close()


def test_build_collector_with_the_wide_knob_builds_device_seaquest(dev, tmp_path):
    col = GS.knob_collector_check(GAME, dev, tmp_path)
    assert tuple(col.envs._state.shape) == (RH.N_ENV, 112)
    col.close()


def test_learn_twice_from_one_seed_is_bit_identical(dev, tmp_path):
    GS.learn_twice_check(GAME, dev, tmp_path)


def test_vector_evaluator_over_the_device_equals_eval_host_on_the_restatement(dev):
    GS.evaluator_run(GAME, dev, minimal_actions=True)


# ---------------------------------------------------------------------------------------------------- resume
def test_state_dict_into_a_fresh_object_continues_bit_identically(dev):
    def lists_travel(a, sd):
        assert tuple(sd["state"].shape) == (6, 112)
        assert sum(len(x) for name in ("e_fish", "e_subs", "divers") for x in a.get_state()[name]) >= 1

    GS.state_dict_run(GAME, dev, np.random.default_rng(4).integers(0, 6, (70, 6)), other="invaders", limit=40, at_snapshot=lists_travel)


def test_learner_save_state_carries_the_environments_through_the_collector_key(dev, tmp_path):
    GS.save_state_check(GAME, dev, tmp_path)
