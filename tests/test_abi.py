"""No GPU needed: the C-ABI library builds for gfx950, loads, and exports every symbol that
include/prism_hip.h declares; argument checking works without touching a device."""
import ctypes
import os
import re

import pytest

from tests import helpers as H


@pytest.fixture(scope="module")
def lib():
    import __graft_entry__ as g
    from prism_amd import _native as N
    if not os.path.exists(N.LIB_PATH):
        g.build()
    return N.lib()


def declared_symbols():
    src = open(os.path.join(H.ROOT, "include", "prism_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(prism_[a-z0-9_]+)\s*\(", src)))


def test_every_declared_symbol_is_exported_and_bound(lib):
    from prism_amd import _native as N
    names = declared_symbols()
    assert len(names) >= 20
    raw = ctypes.CDLL(N.LIB_PATH)
    for n in names:
        assert hasattr(raw, n), f"{n} declared in prism_hip.h but not exported"
        assert n in N.SIGNATURES, f"{n} has no ctypes signature in prism_amd/_native.py"
    assert set(N.SIGNATURES) == set(names)
    assert lib.prism_abi_version() == 3
    # (documentation drift guard: DESIGN.md quotes the number of entry points)
    assert f"({len(names)} entry points)" in open(os.path.join(H.ROOT, "DESIGN.md")).read()


def test_struct_layouts_match_header():
    """ctypes mirrors must have the C sizes (guards against silent field drift)."""
    from prism_amd import _native as N
    assert ctypes.sizeof(N.ReplayDesc) == 8 + 8 + 4 + 4 + 10 * 8 + 16 * 8
    assert ctypes.sizeof(N.ModelDims) == 16 * 4 + 4 * 4 + 4          # (+ squish_fn)
    assert ctypes.sizeof(N.ParamOffsets) == 23 * 8
    assert ctypes.sizeof(N.AdamHyper) == 4 * 8 + 2 * 4
    # learner desc: dims(84 + 4 padding) off(184) batch+embed(8) 6 ptrs, 7 ptrs, 4 ptrs, seed/offset/rng (24), 6 ptrs + size_t + hyper(40), host_status
    assert ctypes.sizeof(N.LearnerDesc) == 88 + 184 + 8 + 6 * 8 + 7 * 8 + 4 * 8 + 24 + 24 + 8 + 8 + 7 * 8 + 8 + 40 + 8
    assert ctypes.sizeof(N.DirectDesc) == 8 + 8 * 8 + 8 * 8 + 8 + 8 + 8 + 8


def test_argument_checks_without_device(lib):
    from prism_amd import _native as N
    assert lib.prism_per_sample(None, 10, 4, None, 0, 0, 0.5, None, None, None) == -1
    assert b"null descriptor" in lib.prism_last_error()
    d = N.ReplayDesc()
    d.capacity, d.tree_capacity = 100, 64
    assert lib.prism_replay_init(ctypes.byref(d), None) == -1
    assert b"tree_capacity" in lib.prism_last_error()
    dims = N.ModelDims()
    assert lib.prism_learner_workspace_bytes(ctypes.byref(dims), 256) == 0          # unsupported dims
    assert lib.prism_learner_supported(ctypes.byref(dims), 256) == -3
    dims.in_channels, dims.n_actions, dims.embed_dim, dims.use_iqn = 4, 6, 1024, 1
    dims.n_basis, dims.iqn_layers, dims.iqn_width, dims.n_tau, dims.n_tau_next, dims.use_layer_norm = 64, 1, 128, 8, 8, 1
    assert lib.prism_learner_supported(ctypes.byref(dims), 256) == 0
    assert lib.prism_learner_workspace_bytes(ctypes.byref(dims), 256) > 8 * 2 ** 20
    assert lib.prism_learner_supported(ctypes.byref(dims), 255) == -3                # B*T not a multiple of 16
    # prism_learner_plan_info: null pointers and a short `out` are refused before anything is written; outside the envelope -3
    n = len(N.PLAN_FIELDS)
    assert n == 9 and "prism_learner_plan_info" in N.SIGNATURES
    out = (ctypes.c_int32 * (n + 1))(*([-77] * (n + 1)))
    assert lib.prism_learner_plan_info(None, 256, 0, out, n) == -1
    assert lib.prism_learner_plan_info(ctypes.byref(dims), 256, 0, None, n) == -1
    assert lib.prism_learner_plan_info(ctypes.byref(dims), 256, 0, out, n - 1) == -1
    assert lib.prism_learner_plan_info(ctypes.byref(dims), 256, 0, out, 0) == -1
    assert lib.prism_learner_plan_info(ctypes.byref(dims), 255, 0, out, n) == -3
    assert lib.prism_learner_plan_info(ctypes.byref(N.ModelDims()), 256, 0, out, n) == -3
    assert list(out) == [-77] * (n + 1)
    dims.propagate_grad = 1
    assert lib.prism_learner_plan_info(ctypes.byref(dims), 256, 2, out, n + 1) == 0      # (a longer `out` is fine: n entries are written)
    # B * T = 2048 at width 128 in bf16x3: iqn_bwd3_kernel with the conv backward inside, 16 slabs, local loss, no heads
    assert list(out) == [2, 0, 1, 16, 1, 0, 1, 0, out[8], -77] and out[8] > 0
    assert lib.prism_learner_plan_info(ctypes.byref(dims), 256, 1, out, n) == 0
    assert list(out)[:8] == [1, 0, out[2], 8, 1, 0, 0, 0] and N.plan_info(dims, 256, "fp32")["bwd"] == "fp32"
    assert N.plan_info(dims, 255) is None


def _fake_learner_desc(lib, cfg_index=2, batch=32):
    """A descriptor every check accepts, over buffers that do not exist (16-byte-aligned made-up addresses): each case of the
    test below breaks ONE condition of it, so the call is refused before anything touches a device."""
    from prism_amd import _native as N
    from prism_amd.agents.hip_agent import model_dims
    from prism_amd.config import baseline_config
    ld = N.LearnerDesc()
    ld.dims = model_dims(baseline_config(cfg_index), 4, 6)
    for f, _ in N.ParamOffsets._fields_:
        setattr(ld.off, f, 0)
    ld.off.n_params = 1 << 20
    ld.batch = batch
    addr = 0x10000000
    for f in ("params", "grads", "adam_m", "adam_v", "adam_step", "obs", "next_obs", "reward", "nonterminal", "gamma", "action",
              "out_td", "out_scalars", "workspace"):
        setattr(ld, f, addr)
        addr += 0x1000000
    if ld.dims.has_target:
        ld.target_params = addr
    ld.workspace_bytes = lib.prism_learner_workspace_bytes(ctypes.byref(ld.dims), batch)
    assert ld.workspace_bytes > 0
    ld.hyper.lr, ld.hyper.beta1, ld.hyper.beta2, ld.hyper.eps = 1e-3, 0.9, 0.999, 1e-8
    ld.hyper.max_grad_norm, ld.hyper.grad_scale = 10.0, 1.0
    rp = N.ReplayDesc()
    rp.capacity, rp.tree_capacity, rp.obs_elems, rp.n_step = 4096, 4096, 100 * ld.dims.in_channels, 3
    return ld, rp


def _set(**fields):
    def edit(ld, rp, opt):
        for k, v in fields.items():
            obj, _, name = k.rpartition("__")
            setattr({"": ld, "dims": ld.dims, "off": ld.off, "rp": rp, "opt": opt}[obj], name, v)
    return edit


# (entry point, configuration, the one edit, return code, text): c3 = IQN alone, c4 = IQN + ten two-layer heads (the two
# Q-head offset checks need a model with heads).  "learner" = prism_learner_fwd_bwd, "opt" = prism_learner_clip_step,
# "back" / "back_opt" / "front" = prism_step_back / prism_step_back_opt / prism_step_front.
REFUSALS = [
    ("learner", 2, None, -1, b"check_learner: null descriptor"),
    ("learner", 2, _set(dims__embed_dim=512), -3, b"model dims / batch not covered by the HIP kernels (need E=1024; IQN: K=64"),
    ("learner", 2, _set(batch=33), -3, b"not covered by the HIP kernels"),
    ("learner", 2, _set(params=None), -1, b"check_learner: null parameter buffers"),
    ("learner", 2, _set(adam_step=None), -1, b"check_learner: null parameter buffers"),
    ("learner", 2, _set(dims__has_target=1), -1, b"check_learner: has_target without target_params"),
    ("learner", 2, lambda ld, rp, opt: setattr(ld, "workspace_bytes", ld.workspace_bytes - 1), -1, b"check_learner: workspace too small"),
    ("learner", 2, _set(workspace=None), -1, b"check_learner: workspace too small"),
    ("learner", 2, lambda ld, rp, opt: setattr(ld, "workspace", ld.workspace + 8), -1, b"check_learner: workspace must be 16-byte aligned"),
    ("learner", 2, lambda ld, rp, opt: setattr(ld, "grads", ld.grads + 4), -1,
     b"check_learner: parameter / gradient / Adam buffers must be 16-byte aligned"),
    ("learner", 2, _set(off__n_params=0), -1, b"check_learner: n_params / phi_w offset alignment"),
    ("learner", 2, _set(off__phi_w=2), -1, b"check_learner: n_params / phi_w offset alignment"),
    ("learner", 2, _set(off__iqn_w1=-1), -1, b"check_learner: IQN parameter offsets missing"),
    ("learner", 2, _set(off__iqn_ln2_g=-1), -1, b"check_learner: IQN parameter offsets missing"),
    ("learner", 3, _set(off__head_base=-1), -1, b"check_learner: Q-head parameter offsets missing"),
    ("learner", 3, _set(off__h_w2=-1), -1, b"check_learner: two-layer Q-head parameter offsets missing"),
    ("learner", 2, _set(obs=None), -1, b"check_learner: null batch arrays"),
    ("learner", 2, _set(action=None), -1, b"check_learner: null batch arrays"),
    ("learner", 2, _set(out_td=None), -1, b"check_learner: null outputs"),
    ("learner", 2, _set(out_scalars=None), -1, b"check_learner: null outputs"),
    ("clip_adam", 2, _set(grads=None), -1, b"check_learner: null parameter buffers"),
    ("opt", 2, None, -1, b"check_opt: null descriptor"),
    ("opt", 2, "null opt", -1, b"check_opt: null optimizer hyper-parameters"),
    ("opt", 2, _set(opt__kind=3), -1, b"check_opt: optimizer kind must be PRISM_OPT_ADAM, PRISM_OPT_RMSPROP or PRISM_OPT_SGD"),
    ("opt", 2, _set(opt__kind=1, fuse_tail=1), -3,
     b"check_opt: the fused tail (fuse_tail != 0) is built for Adam only; pass fuse_tail = 0 with RMSprop / SGD"),
    ("back_opt", 2, _set(opt__kind=2, fuse_tail=1), -3, b"built for Adam only"),
    ("opt", 2, _set(opt__kind=1, out_td=None), -1, b"check_learner: null outputs"),
    ("back", 2, "null rp", -1, b"check_replay_for_step: null replay descriptor"),
    ("front", 2, "null rp", -1, b"check_replay_for_step: null replay descriptor"),
    ("back", 2, _set(rp__obs_elems=300), -1, b"check_replay_for_step: replay obs_elems must equal 10*10*C"),
    ("front", 2, _set(rp__obs_elems=401), -1, b"check_replay_for_step: replay obs_elems must equal 10*10*C"),
    ("back", 2, _set(rp__n_step=0), -1, b"check_replay_for_step: n_step out of range"),
    ("back_opt", 2, _set(rp__n_step=16), -1, b"check_replay_for_step: n_step out of range"),
    ("back", 2, _set(workspace_bytes=16), -1, b"check_learner: workspace too small"),
    ("back", 2, "null index", -1, b"step_back: null index"),
]


@pytest.mark.parametrize("case", range(len(REFUSALS)))
def test_learner_refusals_without_device(lib, case):
    """Every refusal of check_learner, check_opt and check_replay_for_step that needs no device: return code and text.  Each
    call fails a check, so no HIP call is reached."""
    from prism_amd import _native as N
    entry, cfg_index, edit, want_rc, want_text = REFUSALS[case]
    ld, rp = _fake_learner_desc(lib, cfg_index)
    opt = N.OptHyper(kind=N.OPT_ADAM, lr=1e-3, alpha=0.99, eps=1e-8)
    if callable(edit):
        edit(ld, rp, opt)
    p_ld = None if edit is None else ctypes.byref(ld)
    p_opt = None if edit == "null opt" else ctypes.byref(opt)
    p_rp = None if edit == "null rp" else ctypes.byref(rp)
    index = None if edit == "null index" else 0x40000000
    rc = {"learner": lambda: lib.prism_learner_fwd_bwd(p_ld, None),
          "clip_adam": lambda: lib.prism_learner_clip_adam(p_ld, None),
          "opt": lambda: lib.prism_learner_clip_step(p_ld, p_opt, None),
          "back": lambda: lib.prism_step_back(p_ld, p_rp, index, 0.5, 1e-6, None),
          "back_opt": lambda: lib.prism_step_back_opt(p_ld, p_opt, p_rp, index, 0.5, 1e-6, None),
          "front": lambda: lib.prism_step_front(p_ld, p_rp, 100, None, 1, 0, 0.4, index, index, None)}[entry]()
    assert rc == want_rc, (rc, lib.prism_last_error())
    assert want_text in lib.prism_last_error(), lib.prism_last_error()


def test_product_never_imports_oracle_and_has_no_cpu_path():
    import subprocess
    import sys
    root = os.path.join(H.ROOT, "prism_amd")
    for dirpath, _, files in os.walk(root):
        for f in files:
            if f.endswith(".py"):
                txt = open(os.path.join(dirpath, f)).read()
                assert "oracle" not in txt.replace("# oracle", ""), f"{f} references the oracle"
    code = ("import sys; sys.path.insert(0, %r)\n"
            "from prism_amd.config import baseline_config\n"
            "from prism_amd.factory import exp_buffer_factory\n"
            "from prism_amd._native import NativeLibraryError\n"
            "try:\n    exp_buffer_factory.build_exp_buffer(baseline_config(2, device='cpu'))\n"
            "except NativeLibraryError as e:\n    print('LOUD', e)\n" % H.ROOT)
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True)
    assert "LOUD" in out.stdout, out.stdout + out.stderr


@pytest.fixture(scope="module")
def device_isa(tmp_path_factory):
    """gfx950 assembly of the two translation units that hold every kernel: {source name: text}."""
    import shutil
    import subprocess
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("hipcc not available")
    ROOT = H.ROOT
    csrc = os.path.join(ROOT, "prism_amd", "csrc")
    tmp = tmp_path_factory.mktemp("isa")
    out = {}
    for src in ("learner.hip", "replay.hip"):
        o = tmp / (src + ".s")
        subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off",
                        "-I" + os.path.join(ROOT, "include"), "-I" + csrc, "-S", "--cuda-device-only",
                        "-o", str(o), os.path.join(csrc, src)], check=True, timeout=900,
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
        out[src] = o.read_text()
    return out


def test_kernels_use_no_scratch_memory(device_isa):
    """A register array that lands in scratch (private segment) costs a kernel several microseconds per
    launch on this path (it happened three times during development: indexed selects, conditionally
    initialised arrays, kernel-argument structs passed by reference).  Require a zero private segment
    for every kernel."""
    bad = []
    for src, text in device_isa.items():
        for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, re.S):
            seg = re.search(r"\.amdhsa_private_segment_fixed_size (\d+)", m.group(2))
            uses = re.search(r"scratch_(load|store)", text[text.find(m.group(1) + ":"):text.find(".amdhsa_kernel " + m.group(1))])
            if seg and int(seg.group(1)) > 0 and uses:
                bad.append((m.group(1), int(seg.group(1))))
    assert not bad, f"kernels with scratch traffic: {bad}"


def test_release_tickets_drain_every_wave_first(device_isa):
    """Cross-workgroup hand-offs (the conv-partial ticket, the grid barrier of the fused tail) publish data other
    workgroups read once the ticket says so.  The protocol: EVERY wave drains its own stores (s_waitcnt vmcnt(0)), the
    workgroup meets (s_barrier), then one lane draws the ticket (a returning global_atomic_add) -- after writing the L2 back
    (buffer_wbl2) where the data went out through ordinary stores, without where every store was written through (far_store:
    the conv ticket since round 4, the light arrivals of the grid barrier).  A barrier alone only proves the stores were
    issued; hipcc moves or drops the wait unless it is pinned.  Check the emitted ISA: walking back from every ticket that
    has a workgroup barrier in front of it, the last s_waitcnt before that s_barrier waits for vmcnt(0), with no store in
    between."""
    text = device_isa["learner.hip"]
    lines = text.splitlines()
    tickets = [i for i, l in enumerate(lines) if re.search(r"\bglobal_atomic_add(_x2)?\b.*\bsc0\b", l)]
    checked, released, bad = 0, 0, []
    for i in tickets:
        j, wb = i - 1, False
        while j >= 0 and "s_barrier" not in lines[j] and not re.match(r"^\S+:\s*$", lines[j].split(";")[0]) or \
                (j >= 0 and lines[j].startswith(".LBB")):
            wb = wb or "buffer_wbl2" in lines[j]
            j -= 1
        if j < 0 or "s_barrier" not in lines[j]:
            continue          # no workgroup barrier in front of it: a lane's own counter, nothing of the other waves is handed over
        f = i
        while f > 0 and not re.match(r"^_ZN\S+:", lines[f]):
            f -= 1
        if not wb and "iqn_post_kernel" not in lines[f]:
            continue          # a plain counter outside the post launch ("last workgroup advances the step count"): nothing is handed over
        checked += 1
        released += int(wb)
        k, ok = j - 1, False
        while k >= 0:                     # back from the barrier: a vmcnt(0) wait before any memory instruction or label
            ins = lines[k].split(";")[0].strip()
            if ins.startswith("s_waitcnt") and "vmcnt(0)" in ins:
                ok = True
                break
            if re.match(r"(global|buffer|flat|scratch)_", ins) or "s_barrier" in ins or re.match(r"^\S+:$", ins):
                break
            k -= 1
        if not ok:
            bad.append((i + 1, lines[i].strip()))
    assert released >= 2, f"expected the full-release arrivals of the two fused-tail instantiations, found {released}"
    assert checked >= 7, f"expected the conv tickets of five post-kernel forms and the grid barriers, found {checked}"
    assert not bad, f"release tickets whose workgroup barrier is not preceded by a vmcnt(0) drain: {bad}"
