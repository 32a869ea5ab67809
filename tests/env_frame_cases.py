"""The five device games as one table, read by tests/test_env_frame_host.py, tests/test_gpu_env_frame.py and the harness of
the games' own suites (tests/game_suite.py); and the run every configuration of the frame test takes -- the Philox path,
sticky actions, a step limit short enough that the reset branch of the step's tail runs, the full action set and one action
out of range."""
import collections
import importlib

import numpy as np

SEED = 0x5EEDFACE12345
STEPS = 16
SIZES = (1, 5)          # one wave of a workgroup; one whole workgroup and one wave of the next (its other waves have no environment)
KW = dict(sticky_action_prob=0.25, episode_timestep_limit=7, minimal_actions=False)
BAD_ACTION = 2 ** 32 + 1          # out of range in its high half only

# A row: the device class of prism_amd.envs, the module of the host restatement, the host class, the observation shape; then
# what the games' suites vary by --
#   cases                   the module of the case table
#   name, stem              MinAtar/<name>-v1; prism_env_<stem>_reset / _step in env_<stem>.hip
#   minimal, full, refused  the two action counts, and the counts the game's refusal table tries
#   knob                    the configuration attributes that switch the game on for its tests
#   learn_minimal           whether the suite's learner plays the minimal set (-v1) or the full one (-v0)
#   step_draw, reset_draw   the keyword of the given draws of step() / reset(), None where it takes none
#   step_ptrs, reset_ptrs   how many draw pointers the C entry points take
#   seed, philox            the suite's seed; its Philox-path run: n, steps, the environments' keywords, the step at which
#                           environment 1's count is set three below 2^32, and the actions (tests/game_suite.py philox_actions)
#   words_packed            whether the suite holds every state word to the codec's packing of the host's fields (Seaquest:
#                           its lists; the 8-word codecs refuse states their games reach, Asterix's ramp_index of 16 for one)
Game = collections.namedtuple("Game", "device ref host obs_shape cases name stem minimal full refused knob learn_minimal "
                                      "step_draw reset_draw step_ptrs reset_ptrs seed philox words_packed", defaults=(False,))


def _philox(steps, limit, carry_at, actions):
    return dict(n=5, steps=steps, kw=dict(sticky_action_prob=0.25, episode_timestep_limit=limit), carry_at=carry_at, actions=actions)


GAMES = dict(
    breakout=Game("DeviceBreakout", "tests.env_ref", "HostBreakout", (10, 10, 4), "tests.env_cases", "Breakout", "breakout", 3, 6, (4, 0),
                  {}, False, "side", "first_side", 1, 1, SEED, _philox(200, 30, 0, ("track", 3))),
    freeway=Game("DeviceFreeway", "tests.freeway_ref", "HostFreeway", (10, 10, 7), "tests.freeway_cases", "Freeway", "freeway", 3, 6, (4, 0),
                 dict(device_env_games=("Breakout", "Freeway")), True, "speeds", "first_speeds", 1, 1, SEED,
                 _philox(200, 60, 100, ("hold", 2))),          # hold u: tests/test_freeway_host.py shows that the run has a win
    asterix=Game("DeviceAsterix", "tests.asterix_ref", "HostAsterix", (10, 10, 4), "tests.asterix_cases", "Asterix", "asterix", 5, 6, (4, 0, 3),
                 dict(device_env_games=("Breakout", "Freeway", "Asterix")), True, "spawn", None, 1, 0, SEED,
                 _philox(300, 60, 150, ("randint", 7, 5))),
    invaders=Game("DeviceSpaceInvaders", "tests.invaders_ref", "HostSpaceInvaders", (10, 10, 6), "tests.invaders_cases", "SpaceInvaders",
                  "invaders", 4, 6, (0, 3, 5, 7), dict(device_env_games=("Breakout", "Freeway", "Asterix", "SpaceInvaders")), True,
                  None, None, 0, 0, SEED, _philox(300, 60, 150, ("randint", 7, 6))),
    seaquest=Game("DeviceSeaquest", "tests.seaquest_ref", "HostSeaquest", (10, 10, 10), "tests.seaquest_cases", "Seaquest", "seaquest", 6, 6,
                  (0, 3, 4, 5, 7), dict(device_env_wide_games=("Seaquest",)), True, "draws", None, 1, 0, 0x5EA0E57C0FFEE,
                  _philox(300, 60, 150, ("randint", 7, 6)), words_packed=True))


def host(game, n):
    """-> (the host restatement of `game` for n environments, its module's assert_same_state)"""
    ref = importlib.import_module(GAMES[game].ref)
    return getattr(ref, GAMES[game].host)(n, SEED, **KW), ref.assert_same_state


def actions(game, n):
    """int64 [STEPS, n] from a seeded RandomState: in [0, 6) but for ONE action of the run.  (The seeds' base is one under
    which every run holds a truncation: Breakout at N = 1 loses its first ball at step 6 under most.)"""
    rng = np.random.RandomState(100 + sorted(GAMES).index(game) * 16 + n)
    acts = rng.randint(0, 6, (STEPS, n)).astype(np.int64)
    acts[rng.randint(STEPS), rng.randint(n)] = BAD_ACTION
    return acts
