"""katome_amd/csrc/counted_key.h -- a two-word record of 33 .. 39 bases with its count (a whole u32) in the free bits of its first
word -- without a GPU (tests/hostshim/counted_key_host.cpp): pack then unpack is the identity, the key and the count do not bleed
into each other, bits 62 and 63 and the bits between key and count stay clear, counted_fits draws the line at 33 and 39 bases, and
the partition digits of a packed record -- HashDigit<2>{48} and {56} of the key taken back out, the group hash >> 48 -- are those of
the plain key, against a mix64 written out here.  (The hash digits themselves do not ride in the word: profiles/count_in_key.md.)"""
import ctypes as C
import itertools
import os
import random
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SRC = os.path.join(HERE, "hostshim", "counted_key_host.cpp")
HDRS = [os.path.join(ROOT, "katome_amd", "csrc", h) for h in ("counted_key.h", "kmer_bits.h")]
u64p = C.POINTER(C.c_uint64)
M64 = (1 << 64) - 1

HB = (2, 8, 14)                                    # key bits in the first word: 33, 36 and 39 bases
COUNTS = (1, 0xFFFF, 0x10000, 0xFFFFFFFF)


def mix64(x):
    x ^= x >> 33; x = x * 0xff51afd7ed558ccd & M64
    x ^= x >> 33; x = x * 0xc4ceb9fe1a85ec53 & M64
    return x ^ (x >> 33)


def hash_key2(w0, w1):
    return mix64(w1 ^ mix64((w0 + 0x9E3779B97F4A7C15) & M64))


@pytest.fixture(scope="module")
def shim():
    so = os.path.join(HERE, "hostshim", "libcounted_key_host.so")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(p) for p in [SRC] + HDRS):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-o", so, SRC])
    lib = C.CDLL(so)
    lib.hs_counted_fits.restype = C.c_int
    lib.hs_counted_fits.argtypes = [C.c_uint32]
    lib.hs_hash_key2.restype = C.c_uint64
    lib.hs_hash_key2.argtypes = [u64p]
    lib.hs_counted_pack.restype = None
    lib.hs_counted_pack.argtypes = [u64p, C.c_uint32, u64p]
    lib.hs_counted_fields.restype = None
    lib.hs_counted_fields.argtypes = [u64p, u64p]
    return lib


def pack(shim, w0, w1, count):
    plain, packed = (C.c_uint64 * 2)(w0, w1), (C.c_uint64 * 2)()
    shim.hs_counted_pack(plain, count, packed)
    return int(packed[0]), int(packed[1])


def fields(shim, p0, p1):
    packed, out = (C.c_uint64 * 2)(p0, p1), (C.c_uint64 * 4)()
    shim.hs_counted_fields(packed, out)
    return [int(v) for v in out]


def keys_of(hb):
    """all key bits clear, all set, and random ones"""
    rng = random.Random(hb)
    yield 0, 0
    yield (1 << hb) - 1, M64
    for _ in range(20):
        yield rng.getrandbits(hb), rng.getrandbits(64)


@pytest.mark.parametrize("hb", HB)
def test_pack_then_unpack_is_the_identity_and_the_top_bits_stay_clear(shim, hb):
    for (w0, w1), count in itertools.product(keys_of(hb), COUNTS):
        p0, p1 = pack(shim, w0, w1, count)
        assert p1 == w1
        assert p0 >> 62 == 0, (hb, hex(w0), count)
        assert fields(shim, p0, p1)[:3] == [w0, w1, count], (hb, hex(w0), hex(w1), count)


@pytest.mark.parametrize("hb", HB)
def test_the_fields_do_not_bleed_into_each_other(shim, hb):
    """key and count in turn at their extremes beside the other at its own: changing one changes only what is read of that one, and
    their bits in the first word are disjoint, with bits 14 .. 29 and 62, 63 clear"""
    top = (1 << hb) - 1
    assert pack(shim, 0, 0, 0) == (0, 0)
    only_key, only_cnt = pack(shim, top, 0, 0)[0], pack(shim, 0, 0, 0xFFFFFFFF)[0]
    assert only_key == top and only_key & only_cnt == 0
    assert only_cnt == 0xFFFFFFFF << 30 and only_cnt >> 62 == 0 and only_cnt & ((1 << 30) - 1) == 0
    assert pack(shim, top, M64, 0xFFFFFFFF)[0] == only_key | only_cnt
    for w0, count in itertools.product((0, top), (0,) + COUNTS):
        assert fields(shim, *pack(shim, w0, 0x0123456789ABCDEF, count))[:3] == [w0, 0x0123456789ABCDEF, count]


def test_counted_fits_33_to_39_bases(shim):
    assert [b for b in range(1, 96) if shim.hs_counted_fits(b)] == list(range(33, 40))
    assert not shim.hs_counted_fits(32) and not shim.hs_counted_fits(40)


@pytest.mark.parametrize("hb", HB)
def test_digits_of_a_packed_record_are_the_hash_digits_of_the_plain_key(shim, hb):
    for w0, w1 in keys_of(hb):
        h = hash_key2(w0, w1)
        assert int(shim.hs_hash_key2((C.c_uint64 * 2)(w0, w1))) == h
        for count in COUNTS:
            got = fields(shim, *pack(shim, w0, w1, count))[3]
            assert got == h and (got >> 48) & 255 == (h >> 48) & 255 and got >> 56 == h >> 56 and got >> 48 == h >> 48
