"""kmer_bits.h rep_orientation, compiled for the host: the orientation the k-mer level's ordered count keys its groups on
(lds_count.hip, lds_count_ordered_kernel) -- runs without a GPU."""
import ctypes as C
import os
import random
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
HDR = os.path.join(os.path.dirname(HERE), "katome_amd", "csrc", "kmer_bits.h")

_SRC = r"""
#include <cstdint>
#include "%s"
using namespace katome;
extern "C" uint64_t rep(uint64_t x, uint32_t k) { Key<1> a; a.w[0] = x; return rep_orientation(a, k).w[0]; }
extern "C" uint64_t rc(uint64_t x, uint32_t k) { Key<1> a; a.w[0] = x; return revcomp(a, k).w[0]; }
"""


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("rep")
    src, so = d / "rep.cpp", d / "librep.so"
    src.write_text(_SRC % HDR)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-o", str(so), str(src)])
    L = C.CDLL(str(so))
    for f in (L.rep, L.rc):
        f.argtypes = [C.c_uint64, C.c_uint32]
        f.restype = C.c_uint64
    return L


def _keys(k, rng):
    m = (1 << (2 * k)) - 1
    edge = [0, m, 0x5555555555555555 & m, 0xAAAAAAAAAAAAAAAA & m, 1, m - 1, 1 << (2 * k - 1), (1 << k) - 1, m ^ ((1 << k) - 1)]
    return edge + [rng.getrandbits(2 * k) for _ in range(2000)]


@pytest.mark.parametrize("k", list(range(3, 32, 2)))
def test_rep_picks_one_orientation_shared_by_both_strands(lib, k):
    rng = random.Random(k)
    for x in _keys(k, rng):
        y = lib.rc(x, k)
        r = lib.rep(x, k)
        assert r in (x, y)                             # one of the two orientations ...
        assert lib.rep(y, k) == r                      # ... the same for both strands
        assert (r >> k) & 1 == 0                       # the high bit of the middle base's code is 0
        assert ((x >> k) & 1) != ((y >> k) & 1)        # (exactly one of the two has it: complement is NOT, the middle base its own mirror)
