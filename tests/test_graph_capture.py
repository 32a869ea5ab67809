"""No GPU needed: every hipGraph capture of the package runs with the cyclic garbage collector held off (destructors of
unreachable agents make HIP calls, which must not land inside a capture), and the collector's state is restored after."""
import contextlib
import gc

import pytest
import torch


@pytest.fixture
def fake_capture(monkeypatch):
    seen = []

    @contextlib.contextmanager
    def graph(g, **kwargs):
        seen.append((g, kwargs, gc.isenabled()))
        yield

    monkeypatch.setattr(torch.cuda, "graph", graph)
    return seen


def test_collector_is_off_inside_a_capture_and_restored_after(fake_capture):
    from prism_amd.agents.hip_agent import graph_capture
    assert gc.isenabled()
    with graph_capture("g", capture_error_mode="thread_local"):
        assert not gc.isenabled()
    assert gc.isenabled()
    assert fake_capture == [("g", {"capture_error_mode": "thread_local"}, False)]
    with pytest.raises(RuntimeError):
        with graph_capture("g"):
            raise RuntimeError("capture failed")
    assert gc.isenabled()


def test_a_disabled_collector_stays_disabled(fake_capture):
    from prism_amd.agents.hip_agent import graph_capture
    gc.disable()
    try:
        with graph_capture("g"):
            pass
        assert not gc.isenabled()
    finally:
        gc.enable()


def test_the_package_captures_only_through_the_helper():
    import os
    from tests import helpers as H
    for dirpath, _, files in os.walk(os.path.join(H.ROOT, "prism_amd")):
        for f in files:
            if f.endswith(".py"):
                src = open(os.path.join(dirpath, f)).read()
                uses = src.count("with torch.cuda.graph(")
                allowed = 1 if f == "hip_agent.py" else 0          # (the helper's own body)
                assert uses == allowed, f"{f}: capture outside graph_capture()"
