"""No GPU, no compile: the five device games stand on one shared frame (csrc/env_frame.h) -- what the frame owns is defined
once and there, every game file includes it, the C ABI of the ten entry points is what it was -- and the run the GPU frame
test takes (tests/env_frame_cases.py) reaches the reset branch of the step's tail on the host restatements alone."""
import os
import re

import numpy as np
import pytest

from tests import env_frame_cases as FC
from tests import helpers as H

CSRC = os.path.join(H.ROOT, "prism_amd", "csrc")
GAME_FILES = ["env_breakout.hip", "env_freeway.hip", "env_asterix.hip", "env_invaders.hip", "env_seaquest.hip"]
# the declarations of include/prism_hip.h as the games' own host tests hold them (white space collapsed)
DECLARATIONS = [
    "int prism_env_breakout_reset(const prism_env_desc *d, const uint8_t *first_side_in, prism_stream_t stream);",
    "int prism_env_breakout_step(const prism_env_desc *d, const int64_t *actions, const double *u_in, const uint8_t *side_in, "
    "int32_t parity, prism_stream_t stream);",
    "int prism_env_freeway_reset(const prism_env_desc *d, const int8_t *first_speeds_in, prism_stream_t stream);",
    "int prism_env_freeway_step(const prism_env_desc *d, const int64_t *actions, const double *u_in, const int8_t *speeds_in, "
    "int32_t parity, prism_stream_t stream);",
    "int prism_env_asterix_reset(const prism_env_desc *d, prism_stream_t stream);",
    "int prism_env_asterix_step(const prism_env_desc *d, const int64_t *actions, const double *u_in, const uint8_t *spawn_in, "
    "int32_t parity, prism_stream_t stream);",
    "int prism_env_invaders_reset(const prism_env_desc *d, prism_stream_t stream);",
    "int prism_env_invaders_step(const prism_env_desc *d, const int64_t *actions, const double *u_in, int32_t parity, "
    "prism_stream_t stream);",
    "int prism_env_seaquest_reset(const prism_env_desc *d, prism_stream_t stream);",
    "int prism_env_seaquest_step(const prism_env_desc *d, const int64_t *actions, const double *u_in, const uint8_t *draws_in, "
    "int32_t parity, prism_stream_t stream);",
]


def _sources():
    return {name: open(os.path.join(CSRC, name)).read() for name in sorted(os.listdir(CSRC)) if name.endswith((".hip", ".h"))}


@pytest.mark.parametrize("what, pattern", [("check_env", r"\bint check_env\s*\("), ("uni", r"\buint32_t uni\s*\(uint32_t"),
                                           ("the argument struct", r"\bstruct EnvArgs\s*\{"),
                                           ("the launch", r"\bint env_launch\s*\("), ("the argument builder", r"\bEnvArgs env_args\s*\(")])
def test_what_the_frame_owns_is_defined_once_and_there(what, pattern):
    found = {name: len(re.findall(pattern, src)) for name, src in _sources().items()}
    assert {name: k for name, k in found.items() if k} == {"env_frame.h": 1}, (what, found)


def test_every_game_includes_the_frame_and_keeps_no_copy():
    src = _sources()
    for name in GAME_FILES:
        assert len(re.findall(r'^#include "env_frame\.h"$', src[name], re.M)) == 1, name
        # no launch-argument struct, no launch and no descriptor check of its own
        assert not re.search(r"\bstruct \w*Args\b", src[name]) and "hipLaunchKernelGGL" not in src[name], name
        assert "__builtin_amdgcn_readfirstlane" not in src[name] and "PRISM_ENV_STATUS_BAD_ACTION" not in src[name], name
        assert len(re.findall(r"\bcheck_env\(d, \d, \"n_actions must be [^\"]+\"\)", src[name])) == 2, name          # its two entry points
    assert sorted(name for name in src if name.startswith("env_") and name.endswith(".hip")) == sorted(GAME_FILES)


def test_the_ten_entry_points_are_declared_as_they_were():
    from prism_amd import _native as N
    header = " ".join(open(os.path.join(H.ROOT, "include", "prism_hip.h")).read().split())
    for decl in DECLARATIONS:
        name = re.match(r"int (\w+)\(", decl).group(1)
        assert decl in header and header.count(name + "(") == 1, name
        assert name in N.SIGNATURES
    games = [re.match(r"env_(\w+)\.hip", name).group(1) for name in GAME_FILES]
    assert sorted(re.match(r"int (\w+)\(", d).group(1) for d in DECLARATIONS) == sorted(f"prism_env_{g}_{e}" for g in games for e in ("reset", "step"))
    # and defined with those parameters, once, in the game's own file
    src = _sources()
    for decl in DECLARATIONS:
        name = re.match(r"int (\w+)\(", decl).group(1)
        body = " ".join(src[f"env_{name.split('_')[2]}.hip"].split())
        assert body.count('extern "C" ' + decl[:-len("prism_stream_t stream);")] + "prism_stream_t stream_) {") == 1, name


@pytest.mark.parametrize("n", FC.SIZES)
@pytest.mark.parametrize("game", sorted(FC.GAMES))
def test_the_frame_run_reaches_a_truncation_and_a_bad_action_on_the_host(game, n):
    """episode_timestep_limit = 7 ends every episode by its 7th step: 16 steps hold at least two episode ends per
    environment, and a truncation among them."""
    host, _ = FC.host(game, n)
    host.reset()
    acts = FC.actions(game, n)
    assert acts.shape == (FC.STEPS, n) and int(((acts < 0) | (acts >= 6)).sum()) == 1
    done, trunc = np.zeros(n, np.int64), np.zeros(n, np.int64)
    for a in acts:
        _, _, d, t = host.step(a)
        assert not (np.asarray(d) & np.asarray(t)).any()
        done, trunc = done + np.asarray(d), trunc + np.asarray(t)
    assert (done + trunc >= 2).all() and trunc.sum() >= 1, (done, trunc)
    assert host.bad_action and host.n_actions == 6
