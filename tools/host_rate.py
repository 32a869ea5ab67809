"""Host-side rates of the learner loop.

    python tools/host_rate.py                      enqueue / total time of Learner.step() + a cProfile of it (c1)
    python tools/host_rate.py --mode ingest        one env step's ingestion for N streams: extend() x N + flush() against
                                                   extend_batch(), host float32 and uint8 arrays, and the whole loop
                                                   collector -> Agent.forward -> ingest -> Learner.step() both ways; where
                                                   the tree has it, extend_batch() once more with the reward clamp and
                                                   the episode bookkeeping on (prism_replay_ingest_tracked)
    python tools/host_rate.py --mode snapshot      exact-resume snapshots at the c3 shapes (capacity 100 000, (10, 10, 4), binary
                                                   observations): Learner.save_state / load_state against the reference-format
                                                   HipReplayBuffer.save / load, median seconds of --rounds runs and bytes on disk
    --root DIR    import prism_amd from another checkout (a build of the parent commit: only the per-row path exists there)
    --out FILE    also write the ingest table there
    --untracked-only   ingest mode without the tracked + clamp column: the process then does exactly what a parent-commit
                       process does, for comparing the untracked call across trees
"""
import argparse
import contextlib
import io
import os
import statistics
import sys
import time
import weakref

ap = argparse.ArgumentParser()
ap.add_argument("--mode", choices=("step", "ingest", "snapshot"), default="step")
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ap.add_argument("--out", default=None)
ap.add_argument("--steps", type=int, default=300)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--untracked-only", action="store_true")
args = ap.parse_args()
sys.path.insert(0, os.path.abspath(args.root))
import numpy as np
import torch
from prism_amd.config import baseline_config
from prism_amd.learner import Learner
from prism_amd.synthetic import fill_replay


def make_learner(i, **over):
    cfg = baseline_config(i, device="cuda:0", log_to_wandb=False, **over)
    ln = Learner()
    with contextlib.redirect_stdout(io.StringIO()):
        ln.configure(cfg, obs_shape=(10, 10, 4), n_actions=6)
    ln.time_phases = False
    return ln


def step_mode():
    ln = make_learner(0)     # c1: the shortest GPU step (30 us)
    fill_replay(ln.experience_buffer, ln.experience_buffer.capacity, seed=0)
    for _ in range(200): ln.step()
    torch.cuda.synchronize()
    import cProfile, pstats
    t0 = time.perf_counter()
    for _ in range(3000): ln.step()
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    print(f"enqueue {1e6*(t1-t0)/3000:.1f} us/step, total {1e6*(t2-t0)/3000:.1f} us/step")
    pr = cProfile.Profile(); pr.enable()
    for _ in range(2000): ln.step()
    pr.disable(); torch.cuda.synchronize()
    pstats.Stats(pr).sort_stats("cumulative").print_stats(12)


class VecStub:
    """N lockstep environments' worth of transitions from a small pool of observations (the collector's own cost -- stepping
    environments, building Timestep objects -- is outside every timed window)."""

    def __init__(self, n, dtype, seed=0):
        self.n, self.rng = n, np.random.default_rng(seed)
        self.pool = [(self.rng.random((n, 10, 10, 4)) < 0.1).astype(dtype) for _ in range(8)]
        self.k = 0

    def arrays(self):
        n, rng = self.n, self.rng
        self.k += 1
        done = rng.random(n) < 0.02
        return (self.pool[self.k % 8], self.pool[(self.k + 1) % 8], rng.integers(0, 6, n).astype(np.int32),
                rng.standard_normal(n).astype(np.float32), done, np.zeros(n, np.bool_))

    def timesteps(self, steps, ids):
        """`steps` env steps as linked Timestep chains, the way the reference's collectors hand them to extend()."""
        from prism_amd.experience import Timestep
        cur = [Timestep(id=next(ids), obs=self.pool[0][e]) for e in range(self.n)]
        out = []
        for _ in range(steps):
            obs, nxt, act, rew, done, _ = self.arrays()
            row = []
            for e in range(self.n):
                t, node = cur[e], Timestep(id=next(ids), obs=nxt[e])
                t.obs, t.action, t.reward, t.done, t.truncated = obs[e], int(act[e]), float(rew[e]), bool(done[e]), False
                if not t.done:
                    t.next = weakref.ref(node)
                row.append(t)
                cur[e] = node
            out.append(row)
        return out, cur


def timed(fn, steps):
    """us per env step: host enqueue, and host + device until the queue is empty."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for k in range(steps):
        fn(k)
    t1 = time.perf_counter()
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    return 1e6 * (t1 - t0) / steps, 1e6 * (t2 - t0) / steps


def ingest_mode():
    from prism_amd.experience import HipReplayBuffer
    has_batch = hasattr(HipReplayBuffer, "extend_batch")
    has_track = hasattr(HipReplayBuffer, "track_episodes") and not args.untracked_only
    lines = [f"# ingestion of one env step of N streams, us per env step (median of {args.rounds} interleaved rounds of "
             f"{args.steps} steps): host enqueue / until the device queue is empty",
             f"# extend_batch in this tree: {'yes' if has_batch else 'no (per-row path only)'}",
             f"# tracked + clamp column (track_episodes, reward_clipping_type = dopamine_clamp): {'yes' if has_track else 'no'}",
             "N     obs      extend()xN+flush()        extend_batch()           ratio (total)" +
             ("     tracked + clamp          tracked - untracked (total)" if has_track else "")]
    ids = iter(range(10 ** 12))
    for n in (1, 4, 16, 64, 256):
        for dtype in (np.float32, np.uint8):
            row_buf = HipReplayBuffer(100_000, 32, device="cuda:0", use_per=True)
            bat_buf = HipReplayBuffer(100_000, 32, device="cuda:0", use_per=True)
            if has_track:
                trk_buf = HipReplayBuffer(100_000, 32, device="cuda:0", use_per=True, reward_clipping_type="dopamine_clamp")
                trk_buf.track_episodes(0.9)
            stub = VecStub(n, dtype)
            res = {"row": [], "batch": [], "trk": []}
            for rnd in range(args.rounds + 1):              # round 0 warms the paths up
                ts, keep = stub.timesteps(args.steps, ids)

                def per_row(k):
                    for t in ts[k]:
                        row_buf.extend(t)
                    row_buf.flush()
                r = timed(per_row, args.steps)
                if has_batch:
                    data = [stub.arrays() for _ in range(args.steps)]
                    b = timed(lambda k: bat_buf.extend_batch(*data[k]), args.steps)
                if has_track:
                    t = timed(lambda k: trk_buf.extend_batch(*data[k]), args.steps)
                if rnd:
                    res["row"].append(r)
                    if has_batch:
                        res["batch"].append(b)
                    if has_track:
                        res["trk"].append(t)
            med = lambda v, j: statistics.median(x[j] for x in v)
            r0, r1 = med(res["row"], 0), med(res["row"], 1)
            line = f"{n:<5d} {np.dtype(dtype).name:<8s} {r0:9.1f} / {r1:9.1f}"
            if has_batch:
                b0, b1 = med(res["batch"], 0), med(res["batch"], 1)
                line += f"     {b0:9.1f} / {b1:9.1f}     {r1 / b1:6.2f}x"
            if has_track:
                t0, t1 = med(res["trk"], 0), med(res["trk"], 1)
                spread = max(x[1] for x in res["batch"]) - min(x[1] for x in res["batch"])
                line += f"     {t0:9.1f} / {t1:9.1f}     {t1 - b1:+6.1f} (untracked spread {spread:.1f})"
            lines.append(line)
            print(line, flush=True)
    # the whole loop: stub vector collector -> Agent.forward(obs[N]) -> ingestion -> Learner.step(), c3 (IQN + PER)
    lines.append("# whole loop, c3: collector stub -> Agent.forward(obs[N]) -> ingest -> Learner.step(); us per iteration (total)")
    for n in (8, 64):
        ln = make_learner(2)
        buf, agent = ln.experience_buffer, ln.agent
        fill_replay(buf, min(buf.capacity, 50_000), seed=0)
        stub = VecStub(n, np.float32)
        res = {"row": [], "batch": [], "trk": []}
        if has_track:
            ln_t = make_learner(2, reward_clipping_type="dopamine_clamp")
            buf_t, agent_t = ln_t.experience_buffer, ln_t.agent
            fill_replay(buf_t, min(buf_t.capacity, 50_000), seed=0)
            buf_t.track_episodes(0.9)
        for rnd in range(3):
            ts, keep = stub.timesteps(args.steps, ids)

            def loop_rows(k):
                acts = agent.forward(stub.pool[k % 8]).cpu().numpy()       # the per-row path needs the actions on the host
                for e, t in enumerate(ts[k]):
                    t.action = int(acts[e])
                    buf.extend(t)
                ln.step(n)
            r = timed(loop_rows, args.steps)
            if has_batch:
                data = [stub.arrays() for _ in range(args.steps)]

                def loop_batch(k):
                    obs, nxt, _, rew, done, trunc = data[k]
                    buf.extend_batch(obs, nxt, agent.forward(obs), rew, done, trunc)   # actions stay on the device
                    ln.step(n)
                b = timed(loop_batch, args.steps)
            if has_track:
                def loop_tracked(k):
                    obs, nxt, _, rew, done, trunc = data[k]
                    buf_t.extend_batch(obs, nxt, agent_t.forward(obs), rew, done, trunc)
                    ln_t.step(n)
                t = timed(loop_tracked, args.steps)
            if rnd:
                res["row"].append(r)
                if has_batch:
                    res["batch"].append(b)
                if has_track:
                    res["trk"].append(t)
        line = f"N = {n:<4d} per-row {statistics.median(x[1] for x in res['row']):9.1f}"
        if has_batch:
            line += f"     extend_batch {statistics.median(x[1] for x in res['batch']):9.1f}"
        if has_track:
            line += f"     tracked + clamp {statistics.median(x[1] for x in res['trk']):9.1f}"
        lines.append(line)
        print(line, flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


def dir_bytes(path):
    return sum(os.path.getsize(os.path.join(b, f)) for b, _d, fs in os.walk(path) for f in fs)


def snapshot_mode():
    import shutil
    import tempfile
    ln = make_learner(2)                                  # c3: IQN + PER, capacity 100 000
    buf = ln.experience_buffer
    fill_replay(buf, buf.capacity, seed=0)
    for _ in range(20):
        ln.step()
    torch.cuda.synchronize()
    root = tempfile.mkdtemp(prefix="prism_snapshot_")
    res = {k: [] for k in ("save_state", "load_state", "save", "load")}
    size = {}
    try:
        for rnd in range(args.rounds):
            snap, ref = os.path.join(root, "snap"), os.path.join(root, f"ref{rnd}")
            t0 = time.perf_counter()
            ln.save_state(snap)
            res["save_state"].append(time.perf_counter() - t0)
            size["save_state"] = dir_bytes(snap)
            fresh = make_learner(2)
            t0 = time.perf_counter()
            fresh.load_state(snap)
            torch.cuda.synchronize()
            res["load_state"].append(time.perf_counter() - t0)
            del fresh
            t0 = time.perf_counter()
            buf.save(ref)
            res["save"].append(time.perf_counter() - t0)
            size["save"] = dir_bytes(ref)
            other = make_learner(2).experience_buffer
            t0 = time.perf_counter()
            other.load(ref)
            torch.cuda.synchronize()
            res["load"].append(time.perf_counter() - t0)
            del other
            shutil.rmtree(ref)
            print(f"round {rnd}: " + "  ".join(f"{k} {v[-1]:.3f} s" for k, v in res.items()), flush=True)
    finally:
        shutil.rmtree(root, ignore_errors=True)
    lines = [f"# snapshots at the c3 shapes: ring of {buf.capacity} x (10, 10, 4) binary observations, PER; median of {args.rounds} runs",
             f"Learner.save_state            {statistics.median(res['save_state']):8.3f} s   {size['save_state']:>12d} bytes",
             f"Learner.load_state            {statistics.median(res['load_state']):8.3f} s",
             f"HipReplayBuffer.save (ref.)   {statistics.median(res['save']):8.3f} s   {size['save']:>12d} bytes",
             f"HipReplayBuffer.load (ref.)   {statistics.median(res['load']):8.3f} s"]
    print("\n".join(lines), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    if not torch.cuda.is_available():
        sys.exit("host_rate.py measures on the GPU: no device found")
    {"step": step_mode, "ingest": ingest_mode, "snapshot": snapshot_mode}[args.mode]()
