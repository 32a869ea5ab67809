"""GPU: the PER scalars at the replay ABI away from alpha = beta = 0.5, eps = 1e-8 -- the exact branches of
common.h pow_alpha / pow_neg_beta (alpha == 1, beta == 1, beta == 0) and the general powf branch, none of which the rest of
the suite executes -- against oracle.per_ref.PrioritizedSamplerOracle(capacity, alpha, beta, eps).

Tiny rings (capacity 37: tree of 64 leaves, batch 16; capacity 300: 512 leaves), the calls tests/test_gpu_replay.py makes:
insert (default priority (max + eps) ** alpha), three rounds of sample + prism_per_update with duplicates in the index,
then inserts over the wrap.

Exact branches: every node of both trees, the running maximum, the sampled slots and the IS weights, bit for bit.

General exponents: the C library's and the device's powf are not bound to the same rounding (neither promises correct
rounding), so each leaf is compared with float64 (p + eps) ** alpha and each weight with float64 (leaf / p_min) ** -beta
formed from the device's own fp32 quotient, within 2 fp32 ulps (the worst distance seen is printed).  Then,
exactly: every internal node is the fp32 sum / min of its two children as read back from the device, the running maximum is
the oracle's, and the sampled slots are the oracle's lower-bound scan run over the device's own tree."""
import weakref

import numpy as np
import pytest
import torch

from tests import helpers as H

pytestmark = pytest.mark.gpu
B = 16
EXACT = [(1.0, 1.0, 1e-2), (1.0, 0.0, 1e-8), (0.5, 1.0, 1e-3)]
GENERAL = [(0.7, 0.4, 1e-6), (0.3, 0.9, 1e-2)]
ULP_BOUND = 2.0


@pytest.fixture(scope="module")
def dev():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    return "cuda:0"


def ulp_distance(x, exact):
    """|x - exact| in fp32 units in the last place of `exact` (x: float32 array, exact: float64 array)."""
    exact = np.asarray(exact, np.float64)
    return np.abs(np.asarray(x, np.float32).astype(np.float64) - exact) / np.spacing(np.abs(exact).astype(np.float32)).astype(np.float64)


class Ring:
    """A device ring and its sampler oracle driven side by side."""

    def __init__(self, dev, cap, alpha, beta, eps, exact):
        from oracle import per_ref
        from prism_amd.experience import HipReplayBuffer
        self.buf = HipReplayBuffer(cap, B, device=dev, n_step=3, gamma=0.99, use_per=True, alpha=alpha, beta=beta)
        self.buf.buffer._sampler._eps = float(eps)          # (the attribute every replay call reads its eps from)
        self.smp = per_ref.PrioritizedSamplerOracle(cap, alpha, beta, eps)
        assert self.smp.sum_tree.capacity == self.buf.tree_capacity
        self.cap, self.tc, self.exact = cap, self.buf.tree_capacity, exact
        self.alpha, self.beta, self.eps = (np.float32(x) for x in (alpha, beta, eps))
        self.want = np.zeros(cap, np.float64)               # general exponents: the float64 value of every leaf
        self.rng = np.random.default_rng(cap + int(1000 * alpha) + int(100 * beta))
        self.cur, self.n_in = None, 0
        self.worst = dict(leaf=0.0, weight=0.0)

    def _obs(self):
        return torch.from_numpy((self.rng.random((10, 10, 4)) < 0.1).astype(np.float32))

    def _leaf64(self, p):
        return (np.float32(p) + self.eps).astype(np.float64) ** np.float64(self.alpha)

    def insert(self, n):
        from prism_amd.experience import Timestep
        if self.cur is None:
            self.cur = Timestep(id=0, obs=self._obs())
        for _ in range(n):
            nxt = Timestep(id=self.cur.id + 1, obs=self._obs())
            self.cur.reward, self.cur.action = float(np.float32(self.rng.standard_normal())), int(self.rng.integers(0, 6))
            self.cur.done, self.cur.truncated = bool(self.n_in % 11 == 10), False
            if not self.cur.done:
                self.cur.next = weakref.ref(nxt)
            slot = self.buf.extend(self.cur)
            assert slot == self.n_in % self.cap
            self.want[slot] = self._leaf64(self.smp.max_priority)
            self.smp.add(slot)
            self.cur, self.n_in = nxt, self.n_in + 1
        self.buf.flush()
        torch.cuda.synchronize()
        self.check_trees("insert")

    def device_trees(self):
        return self.buf.sum_tree.cpu().numpy().copy(), self.buf.min_tree.cpu().numpy().copy()

    def check_trees(self, what):
        s, m = self.device_trees()
        assert np.float32(self.buf.per_state[0].item()) == np.float32(self.smp.max_priority), f"{what}: running maximum"
        if self.exact:
            np.testing.assert_array_equal(s, self.smp.sum_tree.values(), err_msg=f"{what}: sum tree")
            np.testing.assert_array_equal(m[1:], self.smp.min_tree.values()[1:], err_msg=f"{what}: min tree")
            return
        size = len(self.buf)
        leaves = s[self.tc:self.tc + size]
        d = ulp_distance(leaves, self.want[:size])
        self.worst["leaf"] = max(self.worst["leaf"], float(d.max()))
        assert d.max() <= ULP_BOUND, f"{what}: leaf {int(d.argmax())} is {d.max():.2f} ulp from float64 (p + eps) ** alpha"
        np.testing.assert_array_equal(m[self.tc:self.tc + size], leaves, err_msg=f"{what}: min-tree leaves")
        inner = np.arange(1, self.tc)
        np.testing.assert_array_equal(s[inner], s[2 * inner] + s[2 * inner + 1], err_msg=f"{what}: sum-tree internal nodes")
        np.testing.assert_array_equal(m[inner], np.minimum(m[2 * inner], m[2 * inner + 1]), err_msg=f"{what}: min-tree internal nodes")
        # the oracle goes on from the device's own trees
        self.smp.sum_tree.values()[:] = s
        self.smp.min_tree.values()[1:] = m[1:]

    def sample_and_update(self, rnd):
        buf, smp, size = self.buf, self.smp, len(self.buf)
        offset = buf._draws + buf._fused_draws
        _, info = buf.sample(return_info=True)
        torch.cuda.synchronize()
        idx, w = info["index"].cpu().numpy(), info["_weight"].cpu().numpy()
        mass = H.philox_per_mass(buf.seed, offset, B, smp.sum_tree.query(0, size))
        idx_o, w_o, ps_o, pm_o = smp.sample(size, mass)
        np.testing.assert_array_equal(idx, idx_o, err_msg=f"round {rnd}: sampled slots")
        assert np.float32(ps_o) == np.float32(buf.per_state[1].item()) and np.float32(pm_o) == np.float32(buf.per_state[2].item())
        if self.exact:
            np.testing.assert_array_equal(w, w_o, err_msg=f"round {rnd}: IS weights")
        else:
            s, _ = self.device_trees()
            quot = s[self.tc + idx] / np.float32(pm_o)                      # the device's own fp32 quotient
            d = ulp_distance(w, quot.astype(np.float64) ** -np.float64(self.beta))
            self.worst["weight"] = max(self.worst["weight"], float(d.max()))
            assert d.max() <= ULP_BOUND, f"round {rnd}: weight {int(d.argmax())} is {d.max():.2f} ulp from float64 (leaf / p_min) ** -beta"
        # writeback with duplicates (the last one wins); magnitudes that move the running maximum
        up = idx.copy()
        up[1], up[5], up[B - 1] = up[0], up[0], up[2]
        td = (np.abs(self.rng.standard_normal(B)) * (1.0 + rnd)).astype(np.float32)
        td[3] = np.float32(1e-4)
        buf.update_priority(torch.from_numpy(up), torch.from_numpy(td))
        torch.cuda.synchronize()
        smp.update_priority(up, td)
        for slot, p in zip(up, td):
            self.want[slot] = self._leaf64(p)
        self.check_trees(f"round {rnd} writeback")


@pytest.mark.parametrize("cap", [37, 300])
@pytest.mark.parametrize("alpha,beta,eps", EXACT + GENERAL)
def test_per_scalars_at_the_replay_abi(dev, cap, alpha, beta, eps):
    ring = Ring(dev, cap, alpha, beta, eps, exact=(alpha, beta, eps) in EXACT)
    ring.insert(cap - 5)
    for rnd in range(3):
        ring.sample_and_update(rnd)
    ring.insert(12)                     # over the wrap: seven rows are overwritten with the default priority
    ring.sample_and_update(3)
    ring.buf.check_status()
    if not ring.exact:
        print(f"capacity {cap}, (alpha, beta, eps) = {(alpha, beta, eps)}: worst distance from float64, leaves "
              f"{ring.worst['leaf']:.3f} ulp, weights {ring.worst['weight']:.3f} ulp")
