"""No GPU needed: the quota rule of the evaluation bookkeeping, host side.  ``EvalQuotaHost`` (tests/eval_quota_ref.py, the
checker of the device) has no recording to pin it -- the rule is the project's own -- so it is pinned two ways: against a
per-stream walk written here, and at N = 1, with the quota set to the episodes a recorded run finished, against the
reference's fixture ``tests/golden/evaluator_runs.npz``.  Then the argument checks of ``prism_eval_track_quota`` through the
C ABI, the struct mirror, the kernel's private segment, the knob-off objects, and the seeds the GPU tests rest on."""
import contextlib
import ctypes
import os
import re

import numpy as np
import pytest

from tests import eval_quota_ref as QR
from tests import eval_ref as ER
from tests import helpers as H

POOL = np.array([0.0, 1.0, -1.0, 0.5, -0.25, 3.0, -7.5, 0.1, -0.1, 1e-3, 1e6, -123456.0, 0.7, -2.59], np.float32)


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from prism_amd import _native as N
    if not os.path.exists(N.LIB_PATH):
        g.build()
    return N.lib()


def _script(n, steps, seed, p_end=0.12):
    rng = np.random.default_rng(seed)
    kind = np.where(rng.random((steps, n)) < p_end, rng.integers(1, 4, (steps, n)), 0).astype(np.uint8)
    return POOL[rng.integers(0, len(POOL), (steps, n))].astype(np.float64), kind


# ---------------------------------------------------------------------------------------------------- (a) the walk
def _walk(reward, kind, quota, max_calls):
    """Independent of EvalQuotaHost: stream by stream, the first `quota` episodes of that stream's own script (within the
    first max_calls steps), each as (call, row, return, length); then the merge in (call, row) order."""
    steps, n = kind.shape
    per_stream, live_rows = [], 0
    for i in range(n):
        eps, start = [], 0
        for k in range(min(steps, max_calls)):
            if len(eps) == quota:
                break
            live_rows += 1
            if kind[k, i]:
                ret = 0.0
                for r in reward[start:k + 1, i]:
                    ret = float(np.float32(r)) + ret
                eps.append((k, i, ret, k + 1 - start))
                start = k + 1
        per_stream.append(eps)
    merged = sorted(e for eps in per_stream for e in eps)
    return per_stream, merged, live_rows


@pytest.mark.parametrize("n,quota,steps,max_calls", [(1, 3, 80, 10 ** 6), (7, 1, 60, 10 ** 6), (7, 2, 120, 10 ** 6),
                                                     (65, 5, 200, 10 ** 6), (9, 5, 200, 23), (4, 2, 6, 10 ** 6)])
def test_counted_episodes_are_each_streams_first_e_merged_in_call_row_order(n, quota, steps, max_calls):
    reward, kind = _script(n, steps, [n, quota, steps])
    host = QR.EvalQuotaHost(n, quota, max_calls)
    calls = QR.run_script(host, reward, kind)
    per_stream, merged, live_rows = _walk(reward, kind, quota, max_calls)
    assert host.ep_done == [len(e) for e in per_stream]
    assert host.qcounts == [sum(len(e) == quota for e in per_stream), 0]
    np.testing.assert_array_equal(ER.bits64(host.returns()), ER.bits64([e[2] for e in merged]))
    assert host.log_length[:len(merged)] == [e[3] for e in merged]
    assert host.counts == [len(merged), sum(e[3] for e in merged), live_rows, calls]
    met = all(len(e) == quota for e in per_stream)
    if met:                                                   # closed by the call that ended the last counted episode
        assert host.closed() and calls == max(e[0] for e in merged) + 1
        assert host.result()["incomplete_streams"] == 0
    elif calls == max_calls:                                  # closed by the cap
        assert host.closed() and host.result()["incomplete_streams"] == n - host.qcounts[0] > 0
    else:                                                     # the script ran out: still open
        assert not host.closed() and calls == steps
    if host.closed():
        before = host.arrays()
        assert not host.track([np.nan] * n, [1] * n, [1] * n)
        for k, v in host.arrays().items():
            np.testing.assert_array_equal(v, before[k])
    res = host.result()
    assert res["calls"] == calls and res["episodes_per_stream"] == quota and res["timesteps"] == live_rows


def test_a_stream_that_met_its_quota_is_never_looked_at():
    """Stream 1 ends at once; NaN rewards and set flags in its later rows change nothing."""
    host = QR.EvalQuotaHost(3, 1)
    assert host.track([1.0, 2.0, 4.0], [0, 1, 0], [0, 0, 0]) and host.ep_done == [0, 1, 0] and host.qcounts[0] == 1
    assert host.track([1.0, np.nan, 4.0], [0, 1, 0], [0, 1, 0]) and host.counts == [1, 1, 5, 2]
    assert host.track([1.0, np.nan, 4.0], [1, 1, 0], [0, 0, 1]) and host.closed()
    assert host.returns() == [2.0, 3.0, 12.0] and host.counts == [3, 7, 7, 3] and host.stats == [17.0, 157.0, 2.0, 12.0]
    assert host.ep_return == [0.0, 0.0, 0.0] and host.ep_done == [1, 1, 1]


# ---------------------------------------------------------------------------------------------------- (b) the fixture
@pytest.mark.parametrize("name", sorted(ER.fixture_runs()))
def test_quota_k_at_one_stream_reproduces_the_reference_run_that_finished_k_episodes(name):
    r = ER.fixture_runs()[name]
    want = r["ep_rews_bits"].view(np.float64)
    K = len(want)
    assert K >= 1
    host = QR.EvalQuotaHost(1, quota=K)
    calls = QR.run_script(host, r["reward"][:, None], r["kind"][:, None])
    np.testing.assert_array_equal(ER.bits64(host.returns()), r["ep_rews_bits"])
    kth_end = int(np.flatnonzero(r["kind"])[K - 1]) + 1          # the step on which the K-th episode ended
    assert host.closed() and calls == kth_end <= r["timesteps"]
    assert host.result()["timesteps"] == host.counts[2] == host.counts[3] == kth_end
    s = q = 0.0
    for x in want.tolist():          # the recurrences, written out
        s, q = s + x, q + x * x
    np.testing.assert_array_equal(ER.bits64(host.stats), ER.bits64([s, q, want.min(), want.max()]))
    assert host.counts[:2] == [K, kth_end] and host.qcounts == [1, 0] and host.ep_done == [K]
    # and the budget rule's restatement, which the recording pins, holds the same words over the finished episodes
    budget = ER.EvalHost(1, r["horizon"])
    ER.run_script(budget, r["reward"][:, None], r["kind"][:, None])
    np.testing.assert_array_equal(ER.bits64(host.stats), ER.bits64(budget.stats))
    assert host.counts[:2] == budget.counts[:2] and host.log_length[:K] == budget.log_length[:K]
    res, ref = host.result(), budget.result()
    assert {k: res[k] for k in ("episodes", "mean", "std", "min", "max", "mean_length", "returns")} == \
        {k: ref[k] for k in ("episodes", "mean", "std", "min", "max", "mean_length", "returns")}


# ---------------------------------------------------------------------------------------------------- the C ABI
def _descs(ev_edit, q_edit):
    from prism_amd import _native as N
    a = 0x40000000
    d = N.EvalDesc(n_streams=8, log_capacity=4, budget=10, ep_return=a, ep_length=a, log_return=a, log_length=a, stats=a,
                   counts=a, host_counts=None)
    q = N.EvalQuota(quota=2, max_calls=100, ep_done=a, qcounts=a, host_closed=None)
    for k, v in ev_edit.items():
        setattr(d, k, v)
    for k, v in q_edit.items():
        setattr(q, k, v)
    return d, q


# (the one broken argument and text the message must carry): prism_eval_track's, then the quota's own
REFUSALS = [
    (dict(ev=None), b"null descriptor"),
    (dict(n_streams=0), b"n_streams must be in [1, 65536]"),
    (dict(n_streams=65537), b"n_streams must be in [1, 65536]"),
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
    (dict(q=None), b"null quota descriptor"),
    (dict(ep_done=None), b"null quota array"),
    (dict(qcounts=None), b"null quota array"),
    (dict(quota=0), b"quota must be >= 1"),
    (dict(quota=-3), b"quota must be >= 1"),
    (dict(max_calls=0), b"max_calls must be >= 1"),
    (dict(n=0), b"n must equal n_streams"),
    (dict(n=7), b"n must equal n_streams"),
    (dict(n=9), b"n must equal n_streams"),
]


@pytest.mark.parametrize("case", range(len(REFUSALS)))
def test_argument_checks_without_device(lib, case):
    """Each case breaks ONE condition of a call every check accepts, over made-up addresses: it returns before any HIP
    call."""
    from prism_amd import _native as N
    edit, text = REFUSALS[case]
    a = 0x50000000
    call = dict(n=8, reward=a, done=a, truncated=a)
    call.update({k: v for k, v in edit.items() if k in call})
    q_names = {f[0] for f in N.EvalQuota._fields_}
    d, q = _descs({k: v for k, v in edit.items() if k not in call and k not in q_names and k not in ("ev", "q")},
                  {k: v for k, v in edit.items() if k in q_names})
    ev = None if "ev" in edit else ctypes.byref(d)
    qp = None if "q" in edit else ctypes.byref(q)
    rc = lib.prism_eval_track_quota(ev, qp, call["n"], call["reward"], call["done"], call["truncated"], None)
    assert rc == N.PRISM_ERR_INVALID, (rc, lib.prism_last_error())
    assert text in lib.prism_last_error() and b"prism_eval_track_quota" in lib.prism_last_error(), lib.prism_last_error()


_C_TYPES = {"int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "double": ctypes.c_double}


def test_eval_quota_matches_the_header_and_the_symbol_is_bound(lib):
    from prism_amd import _native as N
    src = re.sub(r"/\*.*?\*/", "", open(N.HEADER_PATH).read(), flags=re.S)
    body = re.search(r"typedef struct prism_eval_quota \{(.*?)\} prism_eval_quota;", src, re.S).group(1)
    fields = []
    for decl in filter(None, (x.strip() for x in body.split(";"))):
        m = re.fullmatch(r"(\w+)\s*(\*?)\s*(\w+)", decl)
        fields.append((m.group(3), ctypes.c_void_p if m.group(2) else _C_TYPES[m.group(1)]))

    class FromHeader(ctypes.Structure):
        _fields_ = fields
    assert [f[0] for f in N.EvalQuota._fields_] == [f[0] for f in fields] == ["quota", "max_calls", "ep_done", "qcounts",
                                                                              "host_closed"]
    assert ctypes.sizeof(N.EvalQuota) == ctypes.sizeof(FromHeader) == 8 + 8 + 3 * 8
    for name, _ in fields:
        assert getattr(N.EvalQuota, name).offset == getattr(FromHeader, name).offset, name
    assert hasattr(ctypes.CDLL(N.LIB_PATH), "prism_eval_track_quota")
    sig = N.SIGNATURES["prism_eval_track_quota"][1]
    assert sig[0] == ctypes.POINTER(N.EvalDesc) and sig[1] == ctypes.POINTER(N.EvalQuota) and len(sig) == 7
    assert lib.prism_abi_version() == 3          # additive: the version stays


def test_the_kernel_has_no_private_segment(tmp_path):
    """Read from the code object's metadata of eval_quota.hip: the .amdhsa_private_segment_fixed_size value only."""
    import shutil
    import subprocess
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    csrc = os.path.join(H.ROOT, "prism_amd", "csrc")
    out = tmp_path / "eval_quota.s"
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off",
                    "-I" + os.path.join(H.ROOT, "include"), "-I" + csrc, "-S", "--cuda-device-only", "-o", str(out),
                    os.path.join(csrc, "eval_quota.hip")], check=True, timeout=600, stdout=subprocess.DEVNULL,
                   stderr=subprocess.DEVNULL)
    kernels = dict(re.findall(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", out.read_text(), re.S))
    names = [k for k in kernels if "eval_track_quota_kernel" in k]
    assert len(names) == 1
    assert int(re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", kernels[names[0]]).group(1)) == 0


# ---------------------------------------------------------------------------------------------------- the knob off
@pytest.fixture
def host_torch(monkeypatch, lib):
    """Let EvalTracker build its object over host tensors: no device context, no pinning (neither exists without a GPU).
    Nothing is launched."""
    import torch
    monkeypatch.setattr(torch.cuda, "device", lambda d: contextlib.nullcontext())
    monkeypatch.setattr(torch.Tensor, "pin_memory", lambda self, *a, **kw: self)
    return torch


@pytest.mark.parametrize("cap", [0, 5, 4096])
def test_tracker_with_the_knob_off_builds_the_descriptor_it_builds_today(host_torch, cap):
    from prism_amd import _native as N
    from prism_amd.evals import EvalTracker
    for t in (EvalTracker(9, 77, cap, "cpu"), EvalTracker(9, 77, cap, "cpu", episodes_per_stream=0, max_calls=0)):
        w, d = t._words, t._desc
        assert w.numel() == 8 + cap + (cap + 1) // 2 and t._quota is None and not hasattr(t, "_ep_done")
        assert (d.n_streams, d.log_capacity, d.budget) == (9, cap, 77)
        assert (d.ep_return, d.ep_length) == (t._ep_return.data_ptr(), t._ep_length.data_ptr())
        assert (d.stats, d.counts, d.host_counts) == (w.data_ptr(), w.data_ptr() + 32, t._host_counts.data_ptr())
        assert (d.log_return, d.log_length) == ((w.data_ptr() + 64, w.data_ptr() + 64 + 8 * cap) if cap else (None, None))
        assert t._ep_return.shape == (9,) and t._ep_length.shape == (9,) and t._host_counts.shape == (2,)
    assert bytes(EvalTracker(9, 77, cap, "cpu")._desc)[:16] == bytes(N.EvalDesc(n_streams=9, log_capacity=cap, budget=77))[:16]


def test_tracker_with_the_knob_on_owns_the_quota_arrays(host_torch):
    from prism_amd.evals import EvalTracker
    t = EvalTracker(9, 77, 5, "cpu", episodes_per_stream=3, max_calls=40)
    w, q = t._words, t._quota
    assert w.numel() == 8 + 5 + 3 + 2 and (q.quota, q.max_calls) == (3, 40)
    assert (q.ep_done, q.qcounts, q.host_closed) == (t._ep_done.data_ptr(), w.data_ptr() + 8 * 16, t._host_closed.data_ptr())
    assert t._desc.log_length + 4 * 5 <= q.qcounts and t._ep_done.shape == (9,) and t._host_closed.shape == (1,)
    with pytest.raises(ValueError, match="max_calls"):
        EvalTracker(9, 77, 5, "cpu", episodes_per_stream=3)
    with pytest.raises(ValueError, match="every stream"):
        t.track(np.zeros(8, np.float32), np.zeros(8, bool), np.zeros(8, bool))


class _Agent:
    """What VectorEvaluator's constructor looks at."""
    tau_rng, device = "philox", "cuda:0"

    def __init__(self):
        from prism_amd.agents.action_selectors import GreedyActionSelector
        self.eval_action_selector = GreedyActionSelector()


class _Envs:
    def __init__(self, limit):
        self.episode_timestep_limit = limit


def test_evaluator_state_dict_with_the_knob_off_equals_todays_and_refuses_across_a_changed_quota():
    from prism_amd.evals import VectorEvaluator
    from prism_amd.util import snapshot
    off = VectorEvaluator(_Agent(), None, 500, 100, episodes_per_env=0, max_steps_per_env=None)
    assert off.state_dict() == VectorEvaluator(_Agent(), None, 500, 100).state_dict() == \
        dict(timesteps_since_last_eval="inf", eval_draws=0, evaluations=0, last=None)
    assert (off.episodes_per_env, off.max_steps_per_env) == (0, 0)
    on = VectorEvaluator(_Agent(), _Envs(30), 500, 100, episodes_per_env=3)
    assert on.max_steps_per_env == 90                                             # E x the environments' limit
    assert VectorEvaluator(_Agent(), _Envs(0), 500, 100, episodes_per_env=3).max_steps_per_env == 100      # no limit: the horizon
    assert VectorEvaluator(_Agent(), None, 500, 100, episodes_per_env=3, max_steps_per_env=7).max_steps_per_env == 7
    on.eval_draws, on.evaluations, on.timesteps_since_last_eval = 4096, 2, 16
    on.last = dict(episodes=2, mean=1.5, std=0.5, min=1.0, max=2.0, mean_length=4.5, timesteps=12, returns=[1.0, 2.0], calls=9,
                   incomplete_streams=0, episodes_per_stream=3)
    st = on.state_dict()
    snapshot.check_plain(st)
    assert st == dict(timesteps_since_last_eval=16, eval_draws=4096, evaluations=2, last=on.last, episodes_per_env=3,
                      max_steps_per_env=90)
    twin = VectorEvaluator(_Agent(), _Envs(30), 500, 100, episodes_per_env=3)
    twin.load_state_dict(st)
    assert twin.state_dict() == st
    for other in (off, VectorEvaluator(_Agent(), _Envs(30), 500, 100, episodes_per_env=2),
                  VectorEvaluator(_Agent(), _Envs(30), 500, 100, episodes_per_env=3, max_steps_per_env=91)):
        with pytest.raises(ValueError, match="does not match"):
            other.load_state_dict(st)
    with pytest.raises(ValueError, match="episodes_per_env does not match"):
        on.load_state_dict(off.state_dict())
    with pytest.raises(ValueError, match="max_steps_per_env"):
        VectorEvaluator(_Agent(), _Envs(0), 500, 0, episodes_per_env=3)


# ---------------------------------------------------------------------------------------------------- what the GPU tests rest on
def test_breakout_under_its_step_limit_closes_within_the_default_cap_whatever_the_actions():
    """tests/test_gpu_eval_quota.py evaluates over DeviceBreakout with QUOTA_ENV's seed, step limit and E: every episode ends
    within the limit, so E episodes per stream end within E x limit calls -- the default cap -- under any policy.  Walked
    here on HostBreakout under three policies; the restatement closes with no incomplete stream."""
    from tests.env_ref import HostBreakout
    from tests.quota_cases import QUOTA_ENV
    seed, kw, E = QUOTA_ENV["seed"], QUOTA_ENV["kw"], QUOTA_ENV["episodes"]
    cap = E * kw["episode_timestep_limit"]
    for n in (1, 5, 17):
        for policy in range(3):
            rng = np.random.default_rng([n, policy])
            act = [lambda: np.zeros(n, np.int64), lambda: rng.integers(0, 6, n), lambda: np.full(n, 1 + policy, np.int64)][policy]
            env, host = HostBreakout(n, seed, **kw), QR.EvalQuotaHost(n, E, cap)
            env.reset()
            while not host.closed():
                _, reward, done, trunc = env.step(act())
                host.track(reward, done, trunc)
            res = host.result()
            assert res["incomplete_streams"] == 0 and res["episodes"] == n * E and res["calls"] <= cap
            assert host.ep_done == [E] * n


def test_eval_bias_tool_runs_and_shows_the_bias_of_the_budget_rule():
    """tools/eval_bias.py at a small size: the quota rule's mean sits at the true one, the budget rule's at N = 64 far
    below it."""
    import subprocess
    import sys
    out = subprocess.run([sys.executable, os.path.join(H.ROOT, "tools", "eval_bias.py"), "--horizon", "20000", "--mean-length",
                          "500", "--reps", "10", "--streams", "1", "64", "--json"], capture_output=True, text=True, check=True)
    import json
    rows = {r["n"]: r for r in json.loads(out.stdout.strip().splitlines()[-1])["rows"]}
    assert abs(rows[1]["budget_bias"]) < 0.1 and abs(rows[64]["quota_bias"]) < 0.1
    assert rows[64]["budget_bias"] < -0.3
