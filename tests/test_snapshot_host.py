"""Host: the exact-resume snapshot container and its RNG codecs (prism_amd/util/snapshot.py).  No GPU."""
import os
import random

import numpy as np
import pytest
import torch

from prism_amd.util import snapshot as S


def _parts(k=0):
    return {"a": {"t": torch.arange(12, dtype=torch.float32).view(3, 4) + k, "n": 7 + k, "x": 0.1, "s": "str", "b": True,
                  "none": None, "big": 2 ** 70, "l": [1, 2.5, "z", [torch.tensor([1, 2], dtype=torch.uint8)], {"k": False}],
                  "d": {"inner": {"deep": [torch.zeros(0)]}, 3: "int key"}},
            "b": {"only": torch.tensor([k], dtype=torch.int64)}}


def _same(x, y):
    if torch.is_tensor(x):
        return torch.is_tensor(y) and x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y)
    if isinstance(x, dict):
        return isinstance(y, dict) and list(x.keys()) == list(y.keys()) and all(_same(x[k], y[k]) for k in x)
    if isinstance(x, list):
        return isinstance(y, list) and len(x) == len(y) and all(_same(a, b) for a, b in zip(x, y))
    return type(x) is type(y) and x == y


def test_round_trip_of_nested_plain_data(tmp_path):
    d = tmp_path / "snap"
    S.write_snapshot(d, _parts(), {"compat": {"replay": {"capacity": 96, "gammas": [1.0, 0.99, 0.99 ** 2]}}})
    parts, man = S.read_snapshot(d)
    assert _same(parts, _parts())
    assert man["format"] == 1 and man["parts"] == ["a", "b"]
    assert man["compat"]["replay"] == {"capacity": 96, "gammas": [1.0, 0.99, 0.99 ** 2]}       # floats come back exactly
    only_b, _ = S.read_snapshot(d, ["b"])
    assert list(only_b) == ["b"]
    assert sorted(os.listdir(tmp_path)) == ["snap"]                    # no temporary or .prev directory is left behind
    with pytest.raises(ValueError, match="no part 'c'"):
        S.read_snapshot(d, ["c"])


def test_extra_files_travel_inside_the_snapshot(tmp_path):
    def extra(tmp):
        os.makedirs(os.path.join(tmp, "agent"))
        with open(os.path.join(tmp, "agent", "model.pt"), "w") as f:
            f.write("x")
    S.write_snapshot(tmp_path / "s", _parts(), {}, extra=extra)
    assert (tmp_path / "s" / "agent" / "model.pt").read_text() == "x" and S.is_snapshot(tmp_path / "s")


class _Thing:
    pass


@pytest.mark.parametrize("bad", [_Thing(), np.float64(1.0), np.zeros(3), (1, 2), {1.5: "float key"}, {"deep": [{"x": _Thing()}]}])
def test_anything_but_plain_data_is_refused(tmp_path, bad):
    with pytest.raises(TypeError, match="snapshot"):
        S.write_snapshot(tmp_path / "s", {"a": {"v": bad}}, {})
    assert os.listdir(tmp_path) == []                                   # refused before anything is written


def test_a_part_file_cannot_name_a_class(tmp_path):
    """Parts are read with weights_only=True: a file that pickles an object is refused at load, whoever wrote it."""
    d = tmp_path / "s"
    S.write_snapshot(d, {"a": {"v": 1}}, {})
    torch.save({"v": _Thing()}, d / "a.pt")
    with pytest.raises(Exception, match="(?i)weights_only|unsupported|_Thing"):
        S.read_snapshot(d)


def test_a_directory_without_manifest_is_not_a_snapshot(tmp_path):
    d = tmp_path / "s"
    S.write_snapshot(d, _parts(), {})
    os.remove(d / S.MANIFEST)
    assert not S.is_snapshot(d) and S.latest(d) is None
    with pytest.raises(FileNotFoundError, match="not a snapshot"):
        S.read_snapshot(d)
    with pytest.raises(ValueError, match="not a snapshot"):             # and a foreign directory is never replaced
        S.write_snapshot(d, _parts(), {})
    assert sorted(os.listdir(d)) == ["a.pt", "b.pt"]


def test_an_interrupted_write_leaves_the_previous_snapshot(tmp_path, monkeypatch):
    d = tmp_path / "s"
    S.write_snapshot(d, _parts(0), {"mark": 0})
    real, calls = S._save_part, []

    def cut(part, path):
        calls.append(path)
        if len(calls) == 2:
            raise KeyboardInterrupt("cut before the manifest")
        real(part, path)
    monkeypatch.setattr(S, "_save_part", cut)
    with pytest.raises(KeyboardInterrupt):
        S.write_snapshot(d, _parts(1), {"mark": 1})
    monkeypatch.setattr(S, "_save_part", real)
    assert len(calls) == 2 and all(str(tmp_path / "s.tmp-") in p for p in calls)      # the cut fell inside the write
    assert sorted(os.listdir(tmp_path)) == ["s"]                        # no half snapshot, here or beside it
    parts, man = S.read_snapshot(d)
    assert man["mark"] == 0 and _same(parts, _parts(0))
    # first write interrupted: nothing at dir at all
    monkeypatch.setattr(S, "_save_part", lambda part, path: (_ for _ in ()).throw(OSError("disk full")))
    with pytest.raises(OSError):
        S.write_snapshot(tmp_path / "fresh", _parts(), {})
    assert sorted(os.listdir(tmp_path)) == ["s"]


def test_prev_rotation(tmp_path, monkeypatch):
    d = tmp_path / "s"
    prev = str(d) + S.PREV_SUFFIX
    S.write_snapshot(d, _parts(0), {"mark": 0})
    seen = {}
    real_replace = os.replace

    def spy(src, dst):
        real_replace(src, dst)
        if dst == str(d):              # the new snapshot has just moved into place: the old one must still be there
            seen["prev_mark"] = S.read_snapshot(prev)[1]["mark"]
            seen["new_mark"] = S.read_snapshot(d)[1]["mark"]
        else:                          # the old one has just moved aside: latest() finds it there
            seen["between"] = S.latest(d)
    monkeypatch.setattr(os, "replace", spy)
    S.write_snapshot(d, _parts(1), {"mark": 1})
    monkeypatch.setattr(os, "replace", real_replace)
    assert seen == {"between": prev, "prev_mark": 0, "new_mark": 1}
    assert not os.path.exists(prev) and S.latest(d) == str(d)           # removed only after the new one is in place
    assert _same(S.read_snapshot(d)[0], _parts(1))
    # a crash between the two renames: only .prev is there, and it is what latest() and a later write work with
    real_replace(str(d), prev)
    assert S.latest(d) == prev and S.read_snapshot(S.latest(d))[1]["mark"] == 1
    S.write_snapshot(d, _parts(2), {"mark": 2})
    assert S.latest(d) == str(d) and S.read_snapshot(d)[1]["mark"] == 2 and not os.path.exists(prev)


N_DRAWS = 1000


def test_numpy_codec():
    for rs in (None, np.random.RandomState(5)):
        src = np.random if rs is None else rs
        src.seed(11)
        src.standard_normal(3)                    # (an odd count leaves a cached gaussian behind: has_gauss = 1)
        src.randint(6, size=17)
        st = S.numpy_rng_state(rs)
        S.check_plain(st)
        want = [src.uniform(0, 1, N_DRAWS), src.standard_normal(N_DRAWS), src.randint(1 << 30, size=N_DRAWS)]
        src.seed(99)
        S.set_numpy_rng_state(st, rs)
        got = [src.uniform(0, 1, N_DRAWS), src.standard_normal(N_DRAWS), src.randint(1 << 30, size=N_DRAWS)]
        for a, b in zip(want, got):
            np.testing.assert_array_equal(a, b)


def test_numpy_codec_through_a_file(tmp_path):
    np.random.seed(3)
    np.random.standard_normal(1)
    S.write_snapshot(tmp_path / "s", {"r": {"np": S.numpy_rng_state(), "py": S.python_rng_state(), "t": S.torch_rng_state()}}, {})
    want = np.random.uniform(0, 1, N_DRAWS)
    np.random.seed(4)
    S.set_numpy_rng_state(S.read_snapshot(tmp_path / "s")[0]["r"]["np"])
    np.testing.assert_array_equal(np.random.uniform(0, 1, N_DRAWS), want)


def test_python_codec():
    for r in (None, random.Random(8)):
        src = random if r is None else r
        src.seed(21)
        src.gauss(0, 1)                           # leaves gauss_next behind
        st = S.python_rng_state(r)
        S.check_plain(st)
        want = [src.random() for _ in range(N_DRAWS)] + [src.gauss(0, 1) for _ in range(N_DRAWS)]
        src.seed(0)
        S.set_python_rng_state(st, r)
        assert [src.random() for _ in range(N_DRAWS)] + [src.gauss(0, 1) for _ in range(N_DRAWS)] == want


def test_torch_codec():
    for gen in (None, torch.Generator().manual_seed(4)):
        if gen is None:
            torch.manual_seed(31)
        torch.randn(5, generator=gen)
        st = S.torch_rng_state(gen)
        S.check_plain(st)
        want = [torch.rand(N_DRAWS, generator=gen), torch.randn(N_DRAWS, generator=gen)]
        st_keep = st.clone()
        if gen is None:
            torch.manual_seed(1)
        else:
            gen.manual_seed(1)
        S.set_torch_rng_state(st, gen)
        assert torch.equal(torch.rand(N_DRAWS, generator=gen), want[0])
        assert torch.equal(torch.randn(N_DRAWS, generator=gen), want[1])
        assert torch.equal(st, st_keep)           # the stored state is not the live one


def test_refusals_name_the_field(tmp_path):
    with pytest.raises(ValueError) as e:
        S.check_compat({"capacity": 96, "n_step": 3}, {"capacity": 128, "n_step": 3}, "HipReplayBuffer.load_state")
    msg = str(e.value)
    assert "capacity" in msg and "96" in msg and "128" in msg and "HipReplayBuffer.load_state" in msg
    with pytest.raises(ValueError, match=r"gammas.*0\.99.*0\.9\b"):
        S.check_compat({"gammas": [1.0, 0.99]}, {"gammas": [1.0, 0.9]}, "x")
    with pytest.raises(ValueError, match="use_per.*True.*False"):
        S.check_compat({"use_per": True}, {"use_per": False}, "x")
    with pytest.raises(ValueError, match="n_step.*None.*3"):                # a field the snapshot does not have
        S.check_compat({}, {"n_step": 3}, "x")
    with pytest.raises(ValueError, match="no compatibility record"):
        S.check_compat(None, {"n_step": 3}, "x")
    S.check_compat({"a": 1, "g": [1.0, 0.5], "extra": 9}, {"a": 1, "g": [1.0, 0.5]}, "x")     # equal records pass
    # a snapshot of another format
    d = tmp_path / "s"
    S.write_snapshot(d, {"a": {"v": 1}}, {})
    text = (d / S.MANIFEST).read_text().replace('"format": 1', '"format": 2')
    (d / S.MANIFEST).write_text(text)
    with pytest.raises(ValueError, match="format.*2.*1"):
        S.read_snapshot(d)
