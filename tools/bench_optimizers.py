"""Step time of the flagship configuration (BASELINE.json configs[2]: IQN + PER, B = 256) per optimizer kind, all in the
post + back launch pair replayed from a hipGraph -- the like-for-like form: RMSprop and SGD have no fused tail, so Adam
is measured with fuse_tail off here (and once with it on, the headline form).  GPU box: python tools/bench_optimizers.py"""
import contextlib, io, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from prism_amd.config import baseline_config
from prism_amd.learner import Learner
from prism_amd.synthetic import fill_replay

KINDS = {"adam, fused tail": dict(fuse_tail=True), "adam, post + back": dict(fuse_tail=False),
         "rmsprop, post + back": dict(fuse_tail=False, use_adam=False, use_rmsprop=True),
         "sgd, post + back": dict(fuse_tail=False, use_adam=False, use_rmsprop=False)}
steps, blocks = int(os.environ.get("OPT_STEPS", "2000")), int(os.environ.get("OPT_BLOCKS", "5"))
for name, over in KINDS.items():
    over = dict(over)
    fuse_tail = over.pop("fuse_tail")
    cfg = baseline_config(2, device="cuda:0", experience_replay_capacity=100_000, **over)
    cfg.fuse_tail = fuse_tail
    ln = Learner()
    with contextlib.redirect_stdout(io.StringIO()):
        ln.configure(cfg, obs_shape=(10, 10, 4), n_actions=6)
    fill_replay(ln.experience_buffer, ln.experience_buffer.capacity, seed=0)
    for _ in range(200):
        ln.step()
    torch.cuda.synchronize()
    us = []
    for _ in range(blocks):
        t0 = time.perf_counter()
        for _ in range(steps):
            ln.step()
        torch.cuda.synchronize()
        us.append((time.perf_counter() - t0) / steps * 1e6)
    ln.agent.check_status()
    us.sort()
    print(f"{name:24s} median {us[len(us) // 2]:7.2f} us/step  (min {us[0]:.2f}, max {us[-1]:.2f}; {blocks} blocks of {steps} steps)"
          f"  finite={bool(torch.isfinite(ln.agent.flat).all())}")
