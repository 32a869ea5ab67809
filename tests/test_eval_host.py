"""No GPU needed: the evaluation bookkeeping's host side.  ``EvalHost`` (tests/eval_ref.py, the checker of the device)
against what the live reference's ``SyncAgentEvaluator`` recorded in ``tests/golden/evaluator_runs.npz``, exactly; the
closing rule for several streams; the argument checks of ``prism_eval_track`` through the C ABI; the descriptor mirror; the
kernel's private segment; the evaluator's snapshot state and the checkpoint scan."""
import ctypes
import os
import re

import numpy as np
import pytest

from tests import eval_ref as ER
from tests import helpers as H


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from prism_amd import _native as N
    if not os.path.exists(N.LIB_PATH):
        g.build()
    return N.lib()


RUNS = ["horizon_zero", "on_an_end", "before_an_end", "after_an_end", "long_first_episode", "one_step_episodes",
        "done_and_truncated", "negative_and_fractional"]


def test_the_fixture_holds_the_runs_the_checks_rest_on():
    runs = ER.fixture_runs()
    assert sorted(runs) == sorted(RUNS)
    ends = lambda r: np.flatnonzero(r["kind"]) + 1                    # timesteps at which an episode ends
    for r in runs.values():
        assert r["reward"].dtype == np.float64 and (r["reward"].astype(np.float32).astype(np.float64) == r["reward"]).all()
        assert len(r["ep_rews_bits"]) >= 1 and r["timesteps"] <= len(r["reward"]) <= 700
    r = runs["horizon_zero"]
    assert r["horizon"] == 0 and r["timesteps"] == ends(r)[0] and len(r["ep_rews_bits"]) == 1
    assert runs["on_an_end"]["horizon"] in ends(runs["on_an_end"])
    assert runs["before_an_end"]["horizon"] + 1 in ends(runs["before_an_end"])
    assert runs["after_an_end"]["horizon"] - 1 in ends(runs["after_an_end"])
    for n in ("on_an_end", "before_an_end", "after_an_end"):
        assert runs[n]["timesteps"] == runs[n]["horizon"]
    r = runs["long_first_episode"]
    assert ends(r)[0] > r["horizon"] and r["timesteps"] == ends(r)[0]
    r = runs["one_step_episodes"]
    assert (r["kind"][:r["timesteps"]] != 0).all() and len(r["ep_rews_bits"]) == r["timesteps"] == 12
    k = runs["done_and_truncated"]["kind"][:runs["done_and_truncated"]["timesteps"]]
    assert {1, 2, 3} <= set(k.tolist())
    r = runs["negative_and_fractional"]
    rets = r["ep_rews_bits"].view(np.float64)
    assert (r["reward"] < 0).any() and (r["reward"] % 1 != 0).any() and (rets < 0).any()
    assert (rets.astype(np.float32).astype(np.float64) != rets).any()          # sums float32 could not hold


@pytest.mark.parametrize("name", RUNS)
def test_eval_host_reproduces_the_reference_exactly(name):
    """N = 1: the returned episode returns bit for bit, and the timesteps consumed."""
    r = ER.fixture_runs()[name]
    host = ER.EvalHost(1, r["horizon"])
    steps = ER.run_script(host, r["reward"][:, None], r["kind"][:, None])
    assert steps == host.counts[2] == host.counts[3] == r["timesteps"]
    np.testing.assert_array_equal(ER.bits64(host.returns()), r["ep_rews_bits"])
    res = host.result()
    assert res["episodes"] == len(r["ep_rews_bits"]) and res["timesteps"] == r["timesteps"]
    assert res["min"] == min(host.returns()) and res["max"] == max(host.returns())
    assert res["mean_length"] == (np.flatnonzero(r["kind"][:steps])[-1] + 1) / res["episodes"]     # back to back from step 0
    assert not host.track([1.0], [1], [0]) and host.counts[2] == r["timesteps"]          # closed: takes nothing


def test_closing_rule_with_three_streams_and_a_horizon_not_divisible_by_three():
    """A step contributes 3 timesteps: horizon 10 closes after the 4th call (12 rows) when an episode has ended by then,
    else at the call in which the first one does; the open episodes are dropped."""
    host = ER.EvalHost(3, 10)
    one, no = [1.0, 2.0, 4.0], [0, 0, 0]
    for k in range(3):
        assert host.track(one, [0, 1, 0] if k == 1 else no, no) and not host.closed()
    assert host.counts[:3] == [1, 2, 9]
    assert host.track(one, no, no) and host.closed() and host.counts == [1, 2, 12, 4]
    before = host.arrays()
    assert not host.track(one, [1, 1, 1], no)
    for k, v in host.arrays().items():
        np.testing.assert_array_equal(v, before[k])
    assert host.result()["returns"] == [4.0] and host.ep_return == [4.0, 4.0, 16.0] and host.ep_length == [4, 2, 4]
    # no episode by the horizon: goes on, and closes inside the call that ends the first one -- whose rows are all taken
    host = ER.EvalHost(3, 4)
    for k in range(5):
        assert host.track(one, no, no) and not host.closed()
    assert host.track(one, [0, 0, 1], [1, 0, 0]) and host.closed()
    assert host.counts == [2, 12, 18, 6] and host.returns() == [6.0, 24.0] and host.stats == [30.0, 612.0, 6.0, 24.0]


def _desc(**edit):
    from prism_amd import _native as N
    a = 0x40000000
    d = N.EvalDesc(n_streams=8, log_capacity=4, budget=10, ep_return=a, ep_length=a, log_return=a, log_length=a, stats=a,
                   counts=a, host_counts=None)
    for k, v in edit.items():
        setattr(d, k, v)
    return d


# (the one broken argument and text the message must carry)
REFUSALS = [
    (dict(ev=None), b"null descriptor"),
    (dict(n=0), b"n must be in [1, n_streams]"),
    (dict(n=9), b"n must be in [1, n_streams]"),
    (dict(n_streams=0), b"n_streams must be in [1, 65536]"),
    (dict(n_streams=65537), b"n_streams must be in [1, 65536]"),
    (dict(budget=-1), b"budget must be >= 0"),
    (dict(log_capacity=-1), b"log_capacity must be >= 0"),
    (dict(ep_return=None), b"null evaluation array"),
    (dict(ep_length=None), b"null evaluation array"),
    (dict(stats=None), b"null evaluation array"),
    (dict(counts=None), b"null evaluation array"),
    (dict(log_return=None), b"may be NULL only with log_capacity == 0"),
    (dict(log_length=None), b"may be NULL only with log_capacity == 0"),
    (dict(reward=None), b"null step array"),
    (dict(done=None), b"null step array"),
    (dict(truncated=None), b"null step array"),
]


@pytest.mark.parametrize("case", range(len(REFUSALS)))
def test_argument_checks_without_device(lib, case):
    """Each case breaks ONE condition of a call every check accepts, over made-up addresses: it returns before any HIP
    call."""
    from prism_amd import _native as N
    edit, text = REFUSALS[case]
    a = 0x50000000
    call = dict(n=4, reward=a, done=a, truncated=a)
    desc_edit = {k: v for k, v in edit.items() if k not in call and k != "ev"}
    call.update({k: v for k, v in edit.items() if k in call})
    d = _desc(**desc_edit)
    ev = None if "ev" in edit else ctypes.byref(d)
    rc = lib.prism_eval_track(ev, call["n"], call["reward"], call["done"], call["truncated"], None)
    assert rc == N.PRISM_ERR_INVALID, (rc, lib.prism_last_error())
    assert text in lib.prism_last_error() and b"prism_eval_track" in lib.prism_last_error(), lib.prism_last_error()


_C_TYPES = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "double": ctypes.c_double}


def test_eval_desc_matches_the_header_and_the_symbol_is_bound(lib):
    from prism_amd import _native as N
    src = re.sub(r"/\*.*?\*/", "", open(N.HEADER_PATH).read(), flags=re.S)
    body = re.search(r"typedef struct prism_eval_desc \{(.*?)\} prism_eval_desc;", src, re.S).group(1)
    fields = []
    for decl in filter(None, (x.strip() for x in body.split(";"))):
        m = re.fullmatch(r"(\w+)\s*(\*?)\s*(\w+)", decl)
        fields.append((m.group(3), ctypes.c_void_p if m.group(2) else _C_TYPES[m.group(1)]))

    class FromHeader(ctypes.Structure):
        _fields_ = fields
    assert [f[0] for f in N.EvalDesc._fields_] == [f[0] for f in fields]
    assert ctypes.sizeof(N.EvalDesc) == ctypes.sizeof(FromHeader) == 4 + 4 + 8 + 7 * 8
    for name, _ in fields:
        assert getattr(N.EvalDesc, name).offset == getattr(FromHeader, name).offset, name
    assert hasattr(ctypes.CDLL(N.LIB_PATH), "prism_eval_track")
    assert N.SIGNATURES["prism_eval_track"][1][0] == ctypes.POINTER(N.EvalDesc)
    assert lib.prism_abi_version() == 3


def test_the_kernel_has_no_private_segment(tmp_path):
    """Read from the code object's metadata of eval_track.hip: the .amdhsa_private_segment_fixed_size value only."""
    import shutil
    import subprocess
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    csrc = os.path.join(H.ROOT, "prism_amd", "csrc")
    out = tmp_path / "eval_track.s"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off",
                    "-I" + os.path.join(H.ROOT, "include"), "-I" + csrc, "-S", "--cuda-device-only", "-o", str(out),
                    os.path.join(csrc, "eval_track.hip")], check=True, timeout=600, stdout=subprocess.DEVNULL,
                   stderr=subprocess.DEVNULL)
    kernels = dict(re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", out.read_text(), re.S))
    names = [k for k in kernels if "eval_track_kernel" in k]
    assert len(names) == 1
    assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", kernels[names[0]]).group(1)) == 0


class _Agent:
    """What VectorEvaluator's constructor looks at."""
    tau_rng, device = "philox", "cuda:0"

    def __init__(self):
        from prism_amd.agents.action_selectors import GreedyActionSelector
        self.eval_action_selector = GreedyActionSelector()


def test_evaluator_state_dict_round_trip_with_inf(tmp_path):
    """Plain data (what a snapshot part may hold), ``inf`` before the first evaluation included."""
    import torch
    from prism_amd.evals import VectorEvaluator
    from prism_amd.util import snapshot
    ev = VectorEvaluator(_Agent(), None, 500, 100)
    assert ev.timesteps_since_last_eval == np.inf
    st = ev.state_dict()
    assert st == dict(timesteps_since_last_eval="inf", eval_draws=0, evaluations=0, last=None)
    snapshot.check_plain(st)
    ev.timesteps_since_last_eval, ev.eval_draws, ev.evaluations = 35, 12345, 2
    ev.last = dict(episodes=2, mean=1.5, std=0.5, min=1.0, max=2.0, mean_length=4.5, timesteps=12, returns=[1.0, 2.0])
    st2 = ev.state_dict()
    snapshot.check_plain(st2)
    torch.save({"evaluator": st, "again": st2}, tmp_path / "part.pt")
    back = torch.load(tmp_path / "part.pt", weights_only=True)
    fresh = VectorEvaluator(_Agent(), None, 500, 100)
    fresh.load_state_dict(back["again"])
    assert fresh.state_dict() == st2 and fresh.timesteps_since_last_eval == 35 and fresh.last == ev.last
    fresh.load_state_dict(back["evaluator"])
    assert fresh.timesteps_since_last_eval == np.inf and fresh.state_dict() == st
    fresh.timesteps_since_last_eval += 8                                     # the first maybe_evaluate_agent evaluates
    assert fresh.timesteps_since_last_eval >= fresh.timesteps_between_evaluations


def test_evaluator_refuses_what_it_cannot_isolate_without_a_device():
    from prism_amd.agents.action_selectors import EGreedyActionSelector
    from prism_amd.evals import VectorEvaluator
    a = _Agent()
    a.tau_rng = "torch"
    with pytest.raises(ValueError, match="tau_rng"):
        VectorEvaluator(a, None, 500, 100)
    a = _Agent()
    a.eval_action_selector = EGreedyActionSelector(1.0, 0.1, 100, 0)
    with pytest.raises(ValueError, match="EGreedyActionSelector"):
        VectorEvaluator(a, None, 500, 100)


def test_scan_checkpoints_orders_by_timesteps_and_skips_incomplete_ones(tmp_path, capsys):
    from prism_amd.evals import CheckpointEvaluator, complete_checkpoints

    def make(name, files=("model.pt", "optimizer.pt", "state.pkl")):
        os.makedirs(tmp_path / name / "agent")
        for f in files:
            (tmp_path / name / "agent" / f).write_bytes(b"")
    make("agent_checkpoint_900")
    make("agent_checkpoint_10000")
    make("agent_checkpoint_2000", files=("model.pt", "optimizer.pt"))          # still being written
    make("agent_checkpoint_50", files=("model.pt", "optimizer.pt", "state.pkl", "target_model.pt"))
    make("backup_checkpoint")
    (tmp_path / "agent_checkpoint_77").write_bytes(b"")                        # a file, not a directory
    want = [str(tmp_path / f"agent_checkpoint_{t}") for t in (10000, 900, 50)]          # by number, not by text
    assert complete_checkpoints(str(tmp_path)) == want
    ce = CheckpointEvaluator.__new__(CheckpointEvaluator)                       # (the scan alone: no agent, no device)
    ce.checkpoint_dir, ce.unprocessed_checkpoints, ce.processed_checkpoints = str(tmp_path), [], []
    ce.scan_checkpoints()
    assert ce.unprocessed_checkpoints == want
    ce.processed_checkpoints.append(ce.unprocessed_checkpoints.pop(0))
    (tmp_path / "agent_checkpoint_2000" / "agent" / "state.pkl").write_bytes(b"")
    ce.scan_checkpoints()
    assert ce.unprocessed_checkpoints == [str(tmp_path / f"agent_checkpoint_{t}") for t in (2000, 900, 50)]
    ce.scan_checkpoints()
    assert len(ce.unprocessed_checkpoints) == 3
    assert capsys.readouterr().out.count("Adding new checkpoint") == 4
