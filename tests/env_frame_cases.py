"""What tests/test_env_frame_host.py and tests/test_gpu_env_frame.py share: the five games, and the run every configuration of
the frame test takes -- the Philox path, sticky actions, a step limit short enough that the reset branch of the step's tail
runs, the full action set and one action out of range."""
import importlib

import numpy as np

SEED = 0x5EEDFACE12345
STEPS = 16
SIZES = (1, 5)          # one wave of a workgroup; one whole workgroup and one wave of the next (its other waves have no environment)
KW = dict(sticky_action_prob=0.25, episode_timestep_limit=7, minimal_actions=False)
BAD_ACTION = 2 ** 32 + 1          # out of range in its high half only
# game -> (the device class of prism_amd.envs, the module of the host restatement, the host class, the observation shape)
GAMES = dict(breakout=("DeviceBreakout", "tests.env_ref", "HostBreakout", (10, 10, 4)),
             freeway=("DeviceFreeway", "tests.freeway_ref", "HostFreeway", (10, 10, 7)),
             asterix=("DeviceAsterix", "tests.asterix_ref", "HostAsterix", (10, 10, 4)),
             invaders=("DeviceSpaceInvaders", "tests.invaders_ref", "HostSpaceInvaders", (10, 10, 6)),
             seaquest=("DeviceSeaquest", "tests.seaquest_ref", "HostSeaquest", (10, 10, 10)))


def host(game, n):
    """-> (the host restatement of `game` for n environments, its module's assert_same_state)"""
    ref = importlib.import_module(GAMES[game][1])
    return getattr(ref, GAMES[game][2])(n, SEED, **KW), ref.assert_same_state


def actions(game, n):
    """int64 [STEPS, n] from a seeded RandomState: in [0, 6) but for ONE action of the run.  (The seeds' base is one under
    which every run holds a truncation: Breakout at N = 1 loses its first ball at step 6 under most.)"""
    rng = np.random.RandomState(100 + sorted(GAMES).index(game) * 16 + n)
    acts = rng.randint(0, 6, (STEPS, n)).astype(np.int64)
    acts[rng.randint(STEPS), rng.randint(n)] = BAD_ACTION
    return acts
