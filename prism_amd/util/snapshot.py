"""The on-disk container of an exact-resume snapshot (``Learner.save_state`` / ``HipAgent.save_state`` /
``HipReplayBuffer.save_state``).  Pure host code: imports and runs without a GPU.

A snapshot is a directory::

    <dir>/<part>.pt     one ``torch.save`` file per part, plain data only (tensors, ints, floats, strs, bools, None,
                        lists, dicts with str / int keys): read back with ``weights_only=True``, so no file can name a class
    <dir>/...           what the ``extra`` callback wrote (the agent's reference-layout ``agent/`` directory)
    <dir>/MANIFEST.json written LAST: ``format``, the part names and the compatibility records.  A directory without it
                        is not a snapshot.

Writing goes to a sibling temporary directory, is fsynced, and is moved into place with ``os.replace``.  A snapshot already
at ``dir`` is moved to ``dir + ".prev"`` first and removed only once the new one is in place: a crash at any point leaves
one complete snapshot, at ``dir`` or at ``dir + ".prev"`` (``latest`` finds it).

The RNG codecs turn the state of NumPy's ``MT19937`` generators, Python's ``random``, and torch's CPU / device generators
into plain data and back."""
import json
import os
import random
import shutil

import numpy as np
import torch

FORMAT = 1
MANIFEST = "MANIFEST.json"
PREV_SUFFIX = ".prev"


# ---------------------------------------------------------------------- plain data
def check_plain(obj, where="part"):
    """Raise ``TypeError`` naming the first value under ``obj`` that is not plain data."""
    if obj is None or (isinstance(obj, (bool, int, float, str)) and not isinstance(obj, np.generic)):
        return          # (np.float64 is a float, but pickles as a NumPy scalar: weights_only would refuse the file)
    if torch.is_tensor(obj):
        if type(obj) not in (torch.Tensor, torch.nn.Parameter):
            raise TypeError(f"snapshot: {where} is a tensor subclass ({type(obj).__name__}); store a plain tensor")
        return
    if isinstance(obj, list):
        for i, v in enumerate(obj):
            check_plain(v, f"{where}[{i}]")
        return
    if type(obj) is dict:
        for k, v in obj.items():
            if not isinstance(k, (str, int)) or isinstance(k, bool):
                raise TypeError(f"snapshot: {where} has a key of type {type(k).__name__}; keys must be str or int")
            check_plain(v, f"{where}[{k!r}]")
        return
    raise TypeError(f"snapshot: {where} holds a {type(obj).__module__}.{type(obj).__name__}; parts hold plain data only "
                    "(tensors, ints, floats, strs, bools, None, lists, dicts)")


def _fsync_dir(path):
    fd = os.open(path, os.O_RDONLY)
    try:
        os.fsync(fd)
    finally:
        os.close(fd)


def _fsync_tree(root):
    for base, _dirs, files in os.walk(root):
        for name in files:
            fd = os.open(os.path.join(base, name), os.O_RDONLY)
            try:
                os.fsync(fd)
            finally:
                os.close(fd)
        _fsync_dir(base)


def _save_part(part, path):
    """One part file (the seam the interrupted-write test cuts at)."""
    torch.save(part, path)


def is_snapshot(dir):
    return os.path.isfile(os.path.join(str(dir), MANIFEST))


def latest(dir):
    """The newest complete snapshot a ``write_snapshot(dir, ...)`` left behind: ``dir``, else ``dir + ".prev"`` (a write
    that was cut between its two renames), else None."""
    dir = os.path.abspath(str(dir)).rstrip(os.sep)
    for d in (dir, dir + PREV_SUFFIX):
        if is_snapshot(d):
            return d
    return None


def write_snapshot(dir, parts, manifest, extra=None):
    """Write ``parts`` (name -> dict of plain data) and ``manifest`` (JSON data; ``format`` and ``parts`` are added) as the
    snapshot ``dir``.  ``extra(tmp_dir)``, if given, writes further files into the directory before the manifest does."""
    dir = os.path.abspath(str(dir)).rstrip(os.sep)
    for name, part in parts.items():
        if not isinstance(name, str) or not name or os.sep in name or name.startswith("."):
            raise ValueError(f"snapshot: bad part name {name!r}")
        if type(part) is not dict:
            raise TypeError(f"snapshot: part {name!r} must be a dict")
        check_plain(part, name)
    man = dict(manifest)
    man["format"] = FORMAT
    man["parts"] = sorted(parts)
    text = json.dumps(man, indent=1, sort_keys=True)          # (refuses what JSON cannot hold before anything is written)
    parent = os.path.dirname(dir)
    os.makedirs(parent, exist_ok=True)
    tmp = f"{dir}.tmp-{os.getpid()}"
    if os.path.lexists(tmp):
        shutil.rmtree(tmp)
    os.makedirs(tmp)
    try:
        for name, part in parts.items():
            _save_part(part, os.path.join(tmp, name + ".pt"))
        if extra is not None:
            extra(tmp)
        with open(os.path.join(tmp, MANIFEST), "w") as f:
            f.write(text)
        _fsync_tree(tmp)
    except BaseException:
        shutil.rmtree(tmp, ignore_errors=True)
        raise
    prev = dir + PREV_SUFFIX
    if os.path.lexists(dir):
        if is_snapshot(dir):
            if os.path.lexists(prev):
                shutil.rmtree(prev)
            os.replace(dir, prev)
        elif os.path.isdir(dir) and not os.listdir(dir):
            os.rmdir(dir)
        else:
            shutil.rmtree(tmp, ignore_errors=True)
            raise ValueError(f"snapshot: {dir} exists and is not a snapshot (no {MANIFEST}); refusing to replace it")
    os.replace(tmp, dir)
    _fsync_dir(parent)
    if os.path.lexists(prev):
        shutil.rmtree(prev)
    return dir


def read_manifest(dir):
    dir = str(dir)
    if not is_snapshot(dir):
        raise FileNotFoundError(f"snapshot: {dir} is not a snapshot (no {MANIFEST})")
    with open(os.path.join(dir, MANIFEST)) as f:
        man = json.load(f)
    check_field("format", man.get("format"), FORMAT, "snapshot")
    return man


def read_snapshot(dir, parts=None):
    """``(parts, manifest)`` of the snapshot ``dir``; ``parts``: names to read (default: all the manifest lists)."""
    man = read_manifest(dir)
    names = man["parts"] if parts is None else list(parts)
    out = {}
    for name in names:
        if name not in man["parts"]:
            raise ValueError(f"snapshot: {dir} has no part {name!r} (it holds {man['parts']})")
        out[name] = torch.load(os.path.join(str(dir), name + ".pt"), map_location="cpu", weights_only=True)
    return out, man


# ---------------------------------------------------------------------- compatibility records
def check_field(field, stored, current, what):
    if isinstance(stored, (list, tuple)) or isinstance(current, (list, tuple)):
        same = isinstance(stored, (list, tuple)) and isinstance(current, (list, tuple)) and list(stored) == list(current)
    else:
        same = stored == current and isinstance(stored, bool) == isinstance(current, bool)
    if not same:
        raise ValueError(f"{what}: {field} does not match: the snapshot was written with {field} = {stored!r}, "
                         f"this object has {field} = {current!r}")


def check_compat(stored, current, what):
    """``ValueError`` naming the first field of the record ``current`` whose stored value differs (or is missing)."""
    if not isinstance(stored, dict):
        raise ValueError(f"{what}: the snapshot holds no compatibility record")
    for field, cur in current.items():
        check_field(field, stored.get(field), cur, what)


# ---------------------------------------------------------------------- RNG codecs
def numpy_rng_state(rs=None):
    """The state of a ``np.random.RandomState`` (None: NumPy's global one) as plain data."""
    kind, key, pos, has_gauss, cached = (np.random if rs is None else rs).get_state()
    if kind != "MT19937":
        raise ValueError(f"snapshot: NumPy generator of kind {kind!r}; only MT19937 is handled")
    return {"kind": kind, "key": torch.from_numpy(np.asarray(key).astype(np.int64)), "pos": int(pos),
            "has_gauss": int(has_gauss), "cached_gaussian": float(cached)}


def set_numpy_rng_state(state, rs=None):
    check_field("kind", state["kind"], "MT19937", "NumPy generator state")
    tup = (state["kind"], state["key"].numpy().astype(np.uint32), int(state["pos"]), int(state["has_gauss"]),
           float(state["cached_gaussian"]))
    (np.random if rs is None else rs).set_state(tup)


def python_rng_state(r=None):
    version, internal, gauss_next = (random if r is None else r).getstate()
    return {"version": int(version), "internal": [int(x) for x in internal],
            "gauss_next": None if gauss_next is None else float(gauss_next)}


def set_python_rng_state(state, r=None):
    (random if r is None else r).setstate((int(state["version"]), tuple(int(x) for x in state["internal"]),
                                          state["gauss_next"]))


def torch_rng_state(generator=None):
    """A ``torch.Generator``'s state (None: the global CPU generator) as a plain uint8 tensor."""
    st = torch.get_rng_state() if generator is None else generator.get_state()
    return st.clone()


def set_torch_rng_state(state, generator=None):
    st = state.to("cpu", torch.uint8).contiguous()
    if generator is None:
        torch.set_rng_state(st)
    else:
        generator.set_state(st)


def device_rng_state(device):
    """The default generator of a GPU device (what ``torch.rand(device=...)`` draws from: ``tau_rng = "torch"``)."""
    return torch.cuda.get_rng_state(torch.device(device)).clone()


def set_device_rng_state(state, device):
    torch.cuda.set_rng_state(state.to("cpu", torch.uint8).contiguous(), torch.device(device))
