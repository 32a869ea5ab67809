"""The captured training iteration (``config.captured_loop``): k x (act -> environment step -> ingest) and the fused learner
step as ONE hipGraph replay, where ``Learner._learn`` otherwise issues four host calls per environment step.

Every piece a replay needs keeps its position on the device: the environments' step counters in their state records, the
acting draws in ``rng_counters[2]``, the epsilon-greedy rows in the agent's device word, the observations in two ping-pong
buffers, and the ring cursor in the buffer's two cursor words (``prism_replay_ingest_cursor``).  What the capture bakes by
value alternates with the parity of the ping-pong: two graphs, one per starting parity; the cursor slot of an ingest launch
is the parity of the observation buffer it reads.  While the ring is still filling (``config.graph_while_filling``) the step's
front launch reads the ring's size from the cursor word the last of the k ingest launches wrote, slot ``p0 ^ (k & 1)``
(``prism_step_front_cursor``); at the fill the loop goes over to the form that takes the size by value.  The capture is a
single chain on a single stream: no side stream, no event fork (a graph with parallel branches needs more hardware queues
than a process may have open).

The host mirrors of everything the replay advanced are applied right behind it, by the same routines the eager calls use
(``HipAgent._act_mirror`` / ``_fused_mirror``, ``_DeviceEnv._step_mirror``, ``HipReplayBuffer.extend_cursor_mirror``):
switching the knob off mid-run, an evaluation, a snapshot or a resume see the state the eager loop would have left.
"""
import warnings

import torch

from prism_amd.agents.hip_agent import graph_capture


class CapturedLoop:
    def __init__(self, learner):
        self.learner = learner
        self.failed = None         # why a capture failed: the loop stays eager for good
        self.reason = None         # why the last iteration judged was not a replay (None: it was, or it warmed one up)
        self.judged = False
        self._key = None
        self._graphs = None        # None | "warm" | {starting parity: graph}
        self._bufs = {}            # (environments, n) -> (actions int64, actions int32, float32 observations for byte environments)

    # ------------------------------------------------------------------ conditions
    def check(self):
        """``(reason, None)`` when the next iteration cannot be a replay, else ``(None, (selector, its native key, whether
        the step's front reads the ring's size from the device))``."""
        from prism_amd.agents.action_selectors import EGreedyActionSelector
        from prism_amd.collectors import VectorCollector
        from prism_amd.envs import _DeviceEnv
        ln = self.learner
        agent, buf, col = ln.agent, ln.experience_buffer, ln.timestep_collector
        if self.failed is not None:
            return f"the capture failed ({self.failed}); the loop stays eager", None
        if not (ln.fused and hasattr(agent, "step_fused") and hasattr(buf, "enqueue_extend_cursor")):
            return "the fused step is off (fused_step, or per_mass_rng / tau_rng is not 'philox')", None
        if not ln.hip_graph:
            return "hip_graph is off", None
        if agent.world != 1:
            return "data parallel (world > 1) is not captured", None
        if agent.tau_rng != "philox" or buf.mass_rng != "philox":
            return "tau_rng and per_mass_rng must be 'philox'", None
        if not agent.act_graph:
            return "act_graph is off", None
        if not (isinstance(col, VectorCollector) and isinstance(col.envs, _DeviceEnv)):
            return "the collector is not a VectorCollector over device environments (a host collector cannot be captured)", None
        if agent._is_eval:
            return "the agent is in evaluation mode", None
        sel = agent.action_selector
        if type(sel) is EGreedyActionSelector and not agent.e_greedy_per_env:
            return "epsilon-greedy tosses one host coin per call (e_greedy_per_env is off): a host coin cannot be captured", None
        if agent._B is None:
            agent._prepare(int(agent.config.batch_size))
        n = col.envs.n_envs
        if n > agent._act_cap:
            return f"{n} environments are more than one acting pass takes ({agent._act_cap})", None
        skey = agent._selector_key(sel)
        if skey is None:
            return f"the training selector ({type(sel).__name__}) has no native kernel", None
        if buf._n_staged:
            return "a row staged by extend() is pending", None
        filling = buf._desc is None or buf._size != buf.capacity
        if filling:
            if not ln.graph_while_filling or buf._desc is None:
                return "the ring is not full yet (its size is baked into the step's launches)", None
            why = agent.fill_form(buf)
            if why is not None:
                return f"the ring is not full yet and graph_while_filling does not apply: {why}", None
        return None, (sel, skey, filling)

    # ------------------------------------------------------------------ one iteration
    def _record(self, p0, k, d, skey, bufs, filling=False):
        """Enqueue one iteration that starts at ping-pong parity ``p0`` on the current stream (inside a capture).  ``filling``:
        the step's front reads the ring's size from the cursor word the last ingest launch wrote -- launch j reads slot
        ``p0 ^ (j & 1)`` and writes the other, so behind k launches the count stands in slot ``p0 ^ (k & 1)``."""
        ln = self.learner
        agent, buf, envs = ln.agent, ln.experience_buffer, ln.timestep_collector.envs
        act64, act32, obs32 = bufs
        for j in range(k):
            p = p0 ^ (j & 1)
            obs = envs._obs[p]
            if obs32 is not None:                      # byte observations: the forward reads float32 (as Agent.forward widens)
                obs32.copy_(obs)
            agent._enqueue_act(obs if obs32 is None else obs32, act64, skey, current=j > 0)
            envs._enqueue_step(act64, p)
            act32.copy_(act64)                         # (the ring stores int32 actions: extend_batch's conversion, captured)
            buf.enqueue_extend_cursor(p, obs, envs._next_obs, act32, envs._reward, envs._done, envs._truncated)
        agent._launch_fused(buf, d, cursor_slot=p0 ^ (k & 1) if filling else None)

    def run(self):
        """One training iteration as one replay: the rows it collected, or None when this iteration has to be the eager
        one (a condition fails -- ``reason`` says which --, or the first iteration of a new capture key warms it up)."""
        ln = self.learner
        self.judged = True
        self.reason, plan = self.check()
        if plan is None:
            return None
        sel, skey, filling = plan
        agent, buf, col = ln.agent, ln.experience_buffer, ln.timestep_collector
        envs = col.envs
        n = envs.n_envs
        k = max(1, -(-int(ln.timesteps_per_iteration) // n))
        col._begin(buf)
        if ln.use_per:
            buf.buffer._sampler._beta = 0.5
        with torch.cuda.device(agent.device):
            buf._stream_table(n)
            d = agent._fused_begin(buf)
            ep = buf._ep_return
            # (the cursor form's key carries the form, not a slot: the two graphs, one per starting parity, bake one each)
            key = (agent._fused_key(buf, d, agent.CURSOR_FORM if filling else None), skey, id(sel), id(envs), n, k, agent._B,
                   agent.workspace.data_ptr(), buf._stream_tab.data_ptr(), None if ep is None else ep.data_ptr(), buf._clip)
            if key != self._key:                       # what a capture bakes has changed: this iteration runs eagerly
                self._key, self._graphs = key, "warm"
                return None
            bufs = self._bufs.get((id(envs), n))
            if bufs is None:
                dev, byte_obs = agent.device, envs._obs[0].dtype != torch.float32
                bufs = self._bufs[(id(envs), n)] = (torch.zeros(n, dtype=torch.int64, device=dev), torch.zeros(n, dtype=torch.int32, device=dev),
                                        torch.zeros(envs._obs[0].shape, dtype=torch.float32, device=dev) if byte_obs else None)
            p0 = envs._parity
            # device words an eager call, an evaluation or a restore has left behind: re-seeded before the replay reads them
            agent._seed_act_words(skey, sel)
            buf.seed_cursor(p0)
            if self._graphs == "warm":
                torch.cuda.current_stream().synchronize()
                graphs = {}
                try:
                    for p in (0, 1):
                        graphs[p] = g = torch.cuda.CUDAGraph()
                        with graph_capture(g, capture_error_mode="thread_local"):
                            self._record(p, k, d, skey, bufs, filling)
                except Exception as e:          # noqa: BLE001 -- any capture failure selects the eager loop, for good
                    torch.cuda.synchronize()
                    self.failed, self._graphs = repr(e), None
                    self.reason = self.check()[0]
                    warnings.warn(f"prism_amd: the training iteration could not be captured ({self.failed}); the loop stays eager")
                    return None                        # (a capture only records: nothing of this iteration has run)
                self._graphs = graphs
            self._graphs[p0].replay()
        for j in range(k):
            agent._act_mirror(n, skey, sel)
            envs._step_mirror()
            buf.extend_cursor_mirror(n, p0 ^ (j & 1))
        col._obs = envs.observe()
        col.rows += k * n
        agent._fused_mirror(buf)
        return k * n
