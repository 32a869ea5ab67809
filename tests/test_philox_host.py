"""CPU: the host restatement of the device RNG (tests/helpers.py::philox4x32 and what is built on it) against the
published Philox4x32-10 known-answer vectors, the quantile-sample contract ``philox_taus`` states, and the C++ text of
``prism_amd/csrc/common.h`` itself compiled for the host.  The GPU tests hold every in-kernel draw to these helpers
(tests/test_gpu_rng_streams.py); here the helpers are held to Philox."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import helpers as H

# Random123 kat_vectors, "philox4x32 10": counter words c0..c3, key words k0 k1 -> output words.  The helper takes the
# counter as (ctr = c1:c0, stream = c3:c2) and the key as seed = k1:k0.
KAT = [
    ((0x00000000, 0x00000000, 0x00000000, 0x00000000), (0x00000000, 0x00000000),
     (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff), (0xffffffff, 0xffffffff),
     (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def _pack(lo, hi):
    return (int(hi) << 32) | int(lo)


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_philox4x32_known_answers(ctr, key, want):
    got = H.philox4x32(_pack(key[0], key[1]), np.array([_pack(ctr[0], ctr[1])], dtype=np.uint64), _pack(ctr[2], ctr[3]))
    assert got.dtype == np.uint32 and got.shape == (1, 4)
    assert tuple(int(x) for x in got[0]) == want


def test_philox4x32_is_elementwise_in_the_counter():
    """A vector of counters gives what the counters give one by one (the helpers draw whole batches at once), also
    across the 32-bit carry of the low counter word."""
    seed, stream = 0x0123456789ABCDEF, H.TAU_KEY + 2
    ctr = np.array([0, 1, 0xFFFFFFFF, 0x100000000, 0x1FFFFFFFF, 2 ** 63 + 5], dtype=np.uint64)
    whole = H.philox4x32(seed, ctr, stream)
    for i, c in enumerate(ctr):
        np.testing.assert_array_equal(whole[i], H.philox4x32(seed, np.array([c], dtype=np.uint64), stream)[0])
    assert len({tuple(r) for r in whole.tolist()}) == len(ctr)


def test_unit_float_stays_below_one():
    """24 random bits: the largest word maps to 1 - 2**-24, exactly representable; a 32-bit conversion would round to 1."""
    u = H.u32_to_unit_float(np.array([0, 0xFF, 0x100, 0x80000000, 0xFFFFFF00, 0xFFFFFFFF], dtype=np.uint32))
    assert u.dtype == np.float32
    np.testing.assert_array_equal(u, np.array([0.0, 0.0, 2.0 ** -24, 0.5, 1.0 - 2.0 ** -24, 1.0 - 2.0 ** -24], dtype=np.float32))
    assert float(u.max()) < 1.0


def test_philox_taus_contract():
    seed, off, T, B = 123, 7 * 3 * 8 * 48, 8, 48
    per_stream = [H.philox_taus(seed, off, T, B, sid) for sid in range(4)]
    for sid, tau in enumerate(per_stream):
        assert tau.dtype == np.float32 and tau.shape == (T * B,)
        assert float(tau.min()) >= 0.0 and float(tau.max()) < 1.0
        # the formula, element by element, from the raw words
        for t, b in ((0, 0), (0, B - 1), (3, 17), (T - 1, B - 1)):
            w = H.philox4x32(seed, np.array([off + t * B + b], dtype=np.uint64), 0x54415530 + sid)[0, 0]
            assert tau[t * B + b] == np.float32(int(w) >> 8) * np.float32(2.0 ** -24)
    for i in range(4):
        for j in range(i + 1, 4):
            assert not np.array_equal(per_stream[i], per_stream[j])
            assert (per_stream[i] == per_stream[j]).sum() <= 1          # (24-bit values: a chance hit at most)
    # consecutive offsets are one sequence: the draws of [off, off + n) do not depend on how the range is cut
    whole = H.philox_taus(seed, off, 2 * T, B, 0)
    np.testing.assert_array_equal(whole[:T * B], per_stream[0])
    np.testing.assert_array_equal(whole[T * B:], H.philox_taus(seed, off + T * B, T, B, 0))
    # another seed, another draw; uniform on the whole (a wide band: this guards the scaling, not the generator)
    assert not np.array_equal(H.philox_taus(seed + 1, off, T, B, 0), per_stream[0])
    big = H.philox_taus(seed, 0, 64, 1024, 0)
    assert abs(float(big.mean()) - 0.5) < 0.01 and abs(float(big.var()) - 1.0 / 12.0) < 0.005


_HOST_PROGRAM = r"""
#include "common.h"
#include <cstdlib>
int main(int argc, char **argv) {
    if (argc < 5) return 2;
    const uint64_t seed = strtoull(argv[1], 0, 0), first = strtoull(argv[2], 0, 0), stream = strtoull(argv[3], 0, 0);
    const int n = atoi(argv[4]);
    const prism::Philox ph(seed);
    for (int i = 0; i < n; ++i) {
        uint32_t r[4];
        ph(first + (uint64_t)i, stream, r);
        const float u = prism::u32_to_unit_float(r[0]);
        const double d = prism::u64_to_unit_double(r[0], r[1]);
        uint32_t ub;
        uint64_t db;
        memcpy(&ub, &u, 4);
        memcpy(&db, &d, 8);
        printf("%08x %08x %08x %08x %08x %016llx\n", r[0], r[1], r[2], r[3], ub, (unsigned long long)db);
    }
    return 0;
}
"""


def _hipcc():
    cand = os.environ.get("HIPCC") or shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    return cand if os.path.isfile(cand) and os.access(cand, os.X_OK) else None


def test_common_h_philox_on_the_host_equals_the_helper(tmp_path):
    """``Philox``, ``u32_to_unit_float`` and ``u64_to_unit_double`` of common.h are ``__host__ __device__``: the very text the
    kernels compile, built for the host alone (no device code, no GPU touched) and compared with the Python helpers."""
    hipcc = _hipcc()
    if hipcc is None:
        pytest.skip("no hipcc to compile the host program with")
    src, exe = tmp_path / "philox_host.cpp", tmp_path / "philox_host"
    src.write_text("#include <string.h>\n" + _HOST_PROGRAM)
    subprocess.run([hipcc, "-x", "hip", "--offload-host-only", "-O1", "-std=c++17", "-ffp-contract=off",
                    "-I", os.path.join(H.ROOT, "include"), "-I", os.path.join(H.ROOT, "prism_amd", "csrc"),
                    str(src), "-o", str(exe)], check=True, capture_output=True, text=True, timeout=300)
    n = 2048
    for seed, first, stream in ((123, 0, H.TAU_KEY), (123, 3 * 8 * 256 * 5, H.TAU_KEY + 3),
                                (0xFEDCBA9876543210, 0xFFFFFFFF - 1000, H.TAU_KEY + 1), (7, 2 ** 40 + 11, 0x5045524D)):
        out = subprocess.run([str(exe), str(seed), str(first), str(stream), str(n)], check=True, capture_output=True,
                             text=True, timeout=60).stdout.split()
        words = np.array([int(x, 16) for x in out], dtype=np.uint64).reshape(n, 6)
        ctr = np.uint64(first) + np.arange(n, dtype=np.uint64)
        r = H.philox4x32(seed, ctr, stream)
        np.testing.assert_array_equal(words[:, :4].astype(np.uint32), r)
        np.testing.assert_array_equal(words[:, 4].astype(np.uint32), H.u32_to_unit_float(r[:, 0]).view(np.uint32))
        if H.TAU_KEY <= stream < H.TAU_KEY + 4:
            np.testing.assert_array_equal(words[:, 4].astype(np.uint32),
                                          H.philox_taus(seed, first, 1, n, stream - H.TAU_KEY).view(np.uint32))
        else:
            # the 53-bit form the PER masses are built on (philox_per_mass with p_sum = 1 narrows exactly this to fp32)
            d = words[:, 5].copy().view(np.float64)
            np.testing.assert_array_equal(H.philox_per_mass(seed, first, n, 1.0), d.astype(np.float32))
