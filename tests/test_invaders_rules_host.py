"""No GPU needed: the kernel file's own rule, codec and image functions (``si_step``, ``si_pack`` / ``si_unpack``, ``si_image`` of
csrc/env_invaders.hip are host-and-device code) run on the CPU by the stand-alone program tools/invaders_host_check.hip,
against steps recorded here from the map-form restatement: the whole case table and seeded play.  What the GPU tests compare
on the device is compared here without one."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import helpers as H
from tests import invaders_cases as IC
from tests.invaders_ref import HostSpaceInvaders


def _record(out, host, actions, u=None):
    from prism_amd.envs import pack_invaders_state
    before = pack_invaders_state(host.get_state()).view(np.uint32)
    next_obs, reward, done, trunc = host.step(actions, u=u)
    after = pack_invaders_state(host.get_state()).view(np.uint32)
    for i in range(host.n_envs):
        out.write(" ".join(str(int(v)) for v in before[i]) + f" {int(host.envs[i]['last_action'])} {host.step_limit}\n")
        image = "".join(str(int(v)) for v in next_obs[i].reshape(-1))
        out.write(" ".join(str(int(v)) for v in after[i]) + f" {float(reward[i])} {int(done[i])} {int(trunc[i])} {image}\n")
    return host.n_envs


def test_the_kernel_files_rules_and_image_on_the_host_equal_the_map_form(tmp_path):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    records, count = tmp_path / "records.txt", 0
    with open(records, "w") as out:
        for group, kw in IC.GROUPS.items():
            n = len(IC.group_cases(group))
            host = HostSpaceInvaders(n, 1, **kw)
            state, actions, u = IC.vector(group, n)
            host.set_state(state)
            for k in range(actions.shape[0]):
                count += _record(out, host, actions[k], u[k])
        rng = np.random.default_rng(5)
        for minimal, limit in ((False, 0), (True, 40)):
            host = HostSpaceInvaders(6, 77, sticky_action_prob=0.2, episode_timestep_limit=limit, minimal_actions=minimal)
            host.reset()
            for k in range(250):
                acts = rng.integers(0, host.n_actions, 6)
                for i in range(0, 6, 2):          # half of the cannons fire whenever they can
                    if host.envs[i]["shot_timer"] == 0:
                        acts[i] = host.n_actions - 1
                count += _record(out, host, acts)
            assert host.branches["kill"] >= 20 and host.branches["terminal"] >= 5 and host.branches["turn_at_column_0"] >= 1
    exe = tmp_path / "invaders_host_check"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "-ffp-contract=off", "-I" + os.path.join(H.ROOT, "include"),
                    "-I" + os.path.join(H.ROOT, "prism_amd", "csrc"), "-x", "hip", os.path.join(H.ROOT, "tools", "invaders_host_check.hip"),
                    "-o", str(exe)], check=True, timeout=600, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    run = subprocess.run([str(exe), str(records)], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0 and f"{count} records, 0 mismatches" in run.stdout, run.stdout + run.stderr
