"""SegmentPool::trim (katome_amd/csrc/mem_pool.h) over a fake backend on the host: a live block keeps its front and gives its
tail back where it lies -- what shrink_to_fit (count_routes.hip) does to a level's list instead of copying it."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "hostshim", "mem_pool_trim_host.cpp")
MiB, GiB = 1 << 20, 1 << 30
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-g", "-O1"]
SAN_ENV = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=1", UBSAN_OPTIONS="halt_on_error=1")

_COPIES = [0]


def _shim():
    _COPIES[0] += 1
    so = os.path.join(HERE, "hostshim", "libmem_pool_trim_host_%d_%d.so" % (os.getpid(), _COPIES[0]))      # one pool per library image
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fPIC", "-shared", "-o", so, SRC])
    lib = C.CDLL(so)
    os.unlink(so)
    for name in ("hs_pool_alloc", "hs_pool_trim", "hs_pool_round", "hs_pool_keep", "hs_pool_small"):
        getattr(lib, name).restype = C.c_uint64
    lib.hs_pool_alloc.argtypes = [C.c_uint64, C.c_int]
    lib.hs_pool_free.argtypes = [C.c_uint64, C.c_int]
    lib.hs_pool_trim.argtypes = [C.c_uint64, C.c_uint64]
    lib.hs_pool_round.argtypes = [C.c_uint64]
    return lib


def stats(lib):
    out = (C.c_uint64 * 7)()
    lib.hs_pool_stats(out)
    return dict(zip(("backend", "allocs", "free", "segments", "live", "free_blocks", "syncs"), (int(x) for x in out)))


@pytest.fixture()
def lib():
    return _shim()


def test_kept_block_and_tail_are_disjoint_and_add_up(lib):
    p = lib.hs_pool_alloc(12 * GiB, 0)
    used = 2 * GiB + 345 * MiB + 64
    left = lib.hs_pool_trim(p, used)
    assert left == lib.hs_pool_round(used) and used <= left < 12 * GiB
    s = stats(lib)
    assert s["free_blocks"] == 1 and s["free"] == 12 * GiB - left and s["live"] == 1 and s["allocs"] == 1
    # the tail is what the next request of its size gets: it starts where the kept block ends
    q = lib.hs_pool_alloc(12 * GiB - left, 0)
    assert q == p + left and stats(lib)["allocs"] == 1 and stats(lib)["free"] == 0
    # the kept block, freed afterwards, and the tail give the whole segment back
    assert lib.hs_pool_free(q, 0) == 1 and lib.hs_pool_free(p, 0) == 1
    s = stats(lib)
    assert s["free_blocks"] == 1 and s["free"] == s["backend"] == 12 * GiB and s["live"] == 0
    assert lib.hs_pool_alloc(12 * GiB, 0) == p and stats(lib)["allocs"] == 1


def test_freeing_the_kept_block_gives_the_whole_segment_back(lib):
    p = lib.hs_pool_alloc(4 * GiB, 0)
    assert lib.hs_pool_trim(p, 1 * GiB) == 1 * GiB
    assert lib.hs_pool_free(p, 0) == 1
    s = stats(lib)
    assert s["free_blocks"] == 1 and s["free"] == s["backend"] == 4 * GiB
    lib.hs_pool_release()
    assert stats(lib)["backend"] == 0


def test_a_tail_not_worth_keeping_changes_nothing(lib):
    keep = lib.hs_pool_keep()
    p = lib.hs_pool_alloc(1 * GiB, 0)
    before = stats(lib)
    assert lib.hs_pool_trim(p, 1 * GiB - keep + 2 * MiB) == 1 * GiB        # would free KEEP - 2 MiB
    assert lib.hs_pool_trim(p, 1 * GiB) == 1 * GiB and lib.hs_pool_trim(p, 5 * GiB) == 1 * GiB
    assert stats(lib) == before
    assert lib.hs_pool_trim(p, 1 * GiB - keep) == 1 * GiB - keep           # exactly KEEP: cut
    assert stats(lib)["free"] == keep


def test_a_small_cache_block_is_left_alone(lib):
    small = lib.hs_pool_small()
    p = lib.hs_pool_alloc(small - 4096, 0)
    before = stats(lib)
    assert lib.hs_pool_trim(p, 64) == lib.hs_pool_round(small - 4096)
    assert stats(lib) == before
    # and a large block never shrinks into the small cache's sizes: it keeps at least SMALL
    q = lib.hs_pool_alloc(1 * GiB, 0)
    assert lib.hs_pool_trim(q, 64) == small
    assert lib.hs_pool_free(q, 0) == 1 and lib.hs_pool_alloc(1 * GiB, 0) == q


def test_the_tail_merges_with_a_free_right_neighbour(lib):
    seg = lib.hs_pool_alloc(8 * GiB, 0)
    lib.hs_pool_free(seg, 0)
    a, b = lib.hs_pool_alloc(4 * GiB, 0), lib.hs_pool_alloc(2 * GiB, 0)    # a | b | 2 GiB free
    assert (a, b) == (seg, seg + 4 * GiB) and stats(lib)["free_blocks"] == 1
    lib.hs_pool_free(b, 0)                                                # a | 4 GiB free
    assert stats(lib)["free_blocks"] == 1 and stats(lib)["free"] == 4 * GiB
    assert lib.hs_pool_trim(a, 1 * GiB) == 1 * GiB
    s = stats(lib)
    assert s["free_blocks"] == 1 and s["free"] == 7 * GiB                 # one block of 7 GiB, not 3 + 4
    assert lib.hs_pool_alloc(7 * GiB, 0) == seg + 1 * GiB and stats(lib)["allocs"] == 1


def test_a_live_right_neighbour_stays_where_it_is(lib):
    seg = lib.hs_pool_alloc(8 * GiB, 0)
    lib.hs_pool_free(seg, 0)
    a, b = lib.hs_pool_alloc(4 * GiB, 0), lib.hs_pool_alloc(4 * GiB, 0)
    assert lib.hs_pool_trim(a, 1 * GiB) == 1 * GiB
    assert stats(lib)["free"] == 3 * GiB and stats(lib)["live"] == 2
    c = lib.hs_pool_alloc(3 * GiB, 0)
    assert c == a + 1 * GiB and c + 3 * GiB == b
    for p in (a, c, b):
        assert lib.hs_pool_free(p, 0) == 1
    s = stats(lib)
    assert s["free_blocks"] == 1 and s["free"] == s["backend"] == 8 * GiB


def test_a_tail_taken_on_another_stream_waits_once(lib):
    p = lib.hs_pool_alloc(4 * GiB, 1)
    assert lib.hs_pool_trim(p, 1 * GiB) == 1 * GiB and stats(lib)["syncs"] == 0
    q = lib.hs_pool_alloc(3 * GiB, 1)                                     # the block's own stream: ordered already
    assert q == p + 1 * GiB and stats(lib)["syncs"] == 0
    lib.hs_pool_free(q, 1)
    assert lib.hs_pool_alloc(3 * GiB, 2) == q and stats(lib)["syncs"] == 1   # another stream waits for it, once
    # a tail straight off the trim, taken on another stream
    r = lib.hs_pool_alloc(4 * GiB, 1)
    assert lib.hs_pool_trim(r, 1 * GiB) == 1 * GiB
    assert lib.hs_pool_alloc(3 * GiB, 3) == r + 1 * GiB and stats(lib)["syncs"] == 2


def test_an_unknown_pointer_is_refused(lib):
    p = lib.hs_pool_alloc(2 * GiB, 0)
    before = stats(lib)
    assert lib.hs_pool_trim(12345, 64) == 0 and lib.hs_pool_trim(p + 4096, 64) == 0
    lib.hs_pool_free(p, 0)
    assert lib.hs_pool_trim(p, 64) == 0                                   # freed: not live any more
    assert stats(lib)["free"] == before["backend"]


@pytest.mark.parametrize("seed", range(4))
def test_random_traffic_with_trims(lib, seed):
    rng = np.random.default_rng(seed)
    live = {}
    trimmed = 0
    for step in range(4000):
        r = rng.random()
        if live and (r < 0.35 or len(live) > 60):
            p = list(live)[int(rng.integers(0, len(live)))]
            assert lib.hs_pool_free(p, int(rng.integers(0, 2))) == 1
            del live[p]
        elif live and r < 0.6:
            p = list(live)[int(rng.integers(0, len(live)))]
            keep = int(rng.integers(0, live[p] + 1))
            left = lib.hs_pool_trim(p, keep)
            assert left >= min(keep, live[p])
            if left < live[p]:                 # (left > live[p]: untouched, and a remainder not worth keeping rides along with the block)
                assert left == lib.hs_pool_round(max(keep, lib.hs_pool_small()))
                trimmed += 1
                live[p] = left
        else:
            n = int(rng.choice([64, 4096, 3 * MiB, 9 * MiB, 40 * MiB, 300 * MiB, 2 * GiB, 7 * GiB]) * (0.5 + rng.random()))
            p = lib.hs_pool_alloc(n, int(rng.integers(0, 2)))
            assert p and p not in live
            live[p] = lib.hs_pool_round(n)
        if step % 97 == 0:
            spans = sorted((p, p + n) for p, n in live.items())
            assert all(x[1] <= y[0] for x, y in zip(spans, spans[1:]))      # live blocks stay disjoint
            s = stats(lib)
            assert s["live"] == len(live) and s["segments"] == s["backend"]
            assert s["free"] + sum(live.values()) <= s["segments"]
    assert trimmed > 50
    for p in list(live):
        lib.hs_pool_free(p, 0)
    s = stats(lib)
    assert s["live"] == 0 and s["free"] == s["segments"] == s["backend"]    # everything merged back
    lib.hs_pool_release()
    assert stats(lib)["backend"] == 0


def test_random_traffic_under_asan_and_ubsan(tmp_path):
    """the same bookkeeping as a program of its own with the sanitizers on (host code only): splits, merges and deletes of blocks"""
    # (no skip: every test of this file needs g++ anyway, and a sanitizer runtime that does not build or run is a failure to see)
    exe = os.path.join(str(tmp_path), "mem_pool_trim_selftest")
    subprocess.check_call(["g++", "-std=c++17", "-DMEM_POOL_TRIM_MAIN"] + SAN + [SRC, "-o", exe])
    out = subprocess.check_output([exe, "20000"], env=SAN_ENV, timeout=600).split()
    assert out[0] == b"ok" and int(out[1]) == 20000 and int(out[2]) > 100
